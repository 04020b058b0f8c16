"""GPU: constrained decoding through the public surface -- both wrappers' ``generate`` (uniform, padded, beams on Llama),
``generate_inflight`` and the ``shards`` CLI -- on the tiny models of tests/test_ragged_generate_gpu.py and tests/test_mpt_slots_gpu.py.

The host loop: a stopping criterion that never stops receives, after every token, the ids so far and the RAW logits the token was chosen
from (``generate`` hands its criteria the model's scores).  tests/constrain_ref.py applied to each row's own history and those logits,
then argmax, must give the token ``generate`` chose."""
import functools
import io
import json
import tarfile

import numpy as np
import pytest
import torch

import beam_ref as R
import constrain_ref as CR
import test_mpt_slots_gpu as MG
import test_ragged_generate_gpu as LG
from kernel_util import bits
from llark_amd import ops

pytestmark = pytest.mark.gpu

N = 10


class _Tap:
    """Stopping criterion that records (ids, the step's raw logits) and never stops."""

    def __init__(self):
        self.steps = []

    def __call__(self, ids, scores, **kw):
        self.steps.append((ids.detach().cpu().clone(), scores.detach().float().cpu().clone()))
        return False


@functools.lru_cache(maxsize=None)
def _llama():
    tok = LG._tok()
    return tok, LG._tiny_model(tok, 8, 128)


@functools.lru_cache(maxsize=None)
def _mpt():
    spec, w, _, _ = MG._workload("full")
    return MG._wrapped(spec, w, 4)


def _words_prompt(first, length):
    """BOS + two of the toy words in turn, `length` tokens in all.  The pairs used below are those after which the tiny Llama's PLAIN
    greedy run repeats a bigram within its first six tokens (found with the plain run alone), so that the ban has something to do."""
    tok = LG._tok()
    words = [tok.vocab[w] for w in LG.WORDS]
    return torch.tensor([1] + (words[first:first + 2] * 20)[:length - 1], dtype=torch.int64)


def _llama_rows():
    return [_words_prompt(2, 30), _words_prompt(4, 17)]


def _cases():
    """name -> (model, generate kwargs without constraints, each row's own prompt)"""
    tok, lm = _llama()
    rows = _llama_rows()
    ids, mask = LG._padded(rows, True)
    uni = [rows[0], _words_prompt(14, 30)]
    mm = _mpt()
    audio = [5, 93, 95, 95, 95, 95, 94]
    g = torch.Generator().manual_seed(5)
    aud = torch.randn(2, 4, 64, generator=g)
    mrows = [torch.tensor(audio + [11, 23, 42] * 6), torch.tensor(audio + [7, 60] * 4)]
    mids, mmask = LG._padded(mrows, True)
    muni = [mrows[0], torch.tensor(audio + [31, 8, 77] * 6)]
    return {
        "llama_padded": (lm, dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), max_new_tokens=N, eos_token_id=-1), rows),
        "llama_uniform": (lm, dict(input_ids=torch.stack(uni).cuda(), max_new_tokens=N, eos_token_id=-1), uni),
        "mpt_padded": (mm, dict(input_ids=mids.cuda(), attention_mask=mmask.cuda(), audio_encodings=[a.cuda() for a in aud], max_new_tokens=N), mrows),
        "mpt_uniform": (mm, dict(input_ids=torch.stack(muni).cuda(), audio_encodings=aud.cuda(), max_new_tokens=N), muni),
    }


CASES = ["llama_padded", "llama_uniform", "mpt_padded", "mpt_uniform"]


def _generate(name, **more):
    m, kw, rows = _cases()[name]
    tap = _Tap()
    out = m.generate(**kw, stopping_criteria=[tap], **more)
    return out, tap, rows, kw["input_ids"].shape[1]


def _check_host_loop(tap, rows, S, eos=-1, n=0, words=(), min_new=0, min_len=0, argmax=True):
    """Every token is the argmax of its step's raw logits with -inf at what the reference bans after the row's own history (argmax False:
    it only is none of the banned ones).  Returns the completions."""
    assert len(tap.steps) >= 2
    outs = []
    for b, prompt in enumerate(rows):
        done = False
        for t, (ids, scores) in enumerate(tap.steps):
            assert ids.shape[1] == S + t + 1
            tokn = int(ids[b, S + t])
            if done:
                continue
            hist = prompt.tolist() + ids[b, S:S + t].tolist()
            vocab = scores.shape[-1]
            banned = CR.banned_set(hist, vocab, n=n, words=words, eos=eos, prompt_len=prompt.numel(), min_new=min_new, min_len=min_len)
            assert tokn not in banned, f"row {b} step {t}: token {tokn} is banned after {hist}"
            if argmax:
                want = int(np.argmax(CR.processed_row(scores[b].numpy(), banned)))
                assert tokn == want, f"row {b} step {t}: {tokn} vs the host loop's {want}"
            done = eos >= 0 and tokn == eos
        outs.append(tap.steps[-1][0][b, S:].tolist())
    return outs


def _bigrams(seq):
    return list(zip(seq[:-1], seq[1:]))


@pytest.mark.parametrize("name", CASES)
def test_no_repeat_ngram_equals_a_host_loop(name):
    plain, _, rows, S = _generate(name)
    got, tap, _, _ = _generate(name, no_repeat_ngram_size=2)
    _check_host_loop(tap, rows, S, n=2)
    for b, prompt in enumerate(rows):
        whole = prompt.tolist() + got[b, S:].tolist()
        bg = _bigrams(whole)[len(prompt) - 1:]                     # every bigram that ends in a generated token
        assert not set(bg) & set(_bigrams(prompt.tolist())) and len(set(bg)) == len(bg), f"row {b}: a bigram repeats in {whole}"
    assert got.shape == plain.shape and not torch.equal(got, plain), "no_repeat_ngram_size=2 changed no token of prompts made of repeated words"
    # off in every spelling: the bits of the plain run
    m, kw, _ = _cases()[name]
    off = m.generate(**kw, no_repeat_ngram_size=0, bad_words_ids=[], suppress_tokens=None, min_new_tokens=0, min_length=None)
    assert torch.equal(off, plain)


@pytest.mark.parametrize("name", CASES)
def test_min_new_tokens_holds_the_eos_back(name):
    m, kw, rows = _cases()[name]
    kw = {k: v for k, v in kw.items() if k != "eos_token_id"}
    S = kw["input_ids"].shape[1]
    first = m.generate(**kw, eos_token_id=-1)[:, S].tolist()
    eos = first[0]
    extra = dict(pad_token_id=0) if name.startswith("mpt") else {}
    plain = m.generate(**kw, eos_token_id=eos, **extra)
    assert int(plain[0, S]) == eos                                 # the plain run's row 0 ends on its first token
    tap = _Tap()
    got = m.generate(**kw, eos_token_id=eos, min_new_tokens=4, stopping_criteria=[tap], **extra)
    assert got.shape[1] >= S + 4 and not (got[:, S:S + 4] == eos).any(), f"an EOS among the first four tokens: {got[:, S:].tolist()}"
    _check_host_loop(tap, rows, S, eos=eos, min_new=4)
    # min_length counts the row's own length: the same ban for a row of len_b tokens asked for len_b + 4
    if name.endswith("uniform"):
        again = m.generate(**kw, eos_token_id=eos, min_length=rows[0].numel() + 4, **extra)
        assert torch.equal(again, got)
    else:
        # a padded batch: the shorter row b, min_length = len_b + 4, which lies below the padded width S.  By the row's own length the EOS
        # is banned for its first four tokens; by HF's padded width (S >= min_length) it never would be, and the row would end at once
        b = min(range(len(rows)), key=lambda i: rows[i].numel())
        want = rows[b].numel() + 4
        assert want < S
        tap = _Tap()
        got = m.generate(**kw, eos_token_id=first[b], min_length=want, stopping_criteria=[tap], **extra)
        assert int(m.generate(**kw, eos_token_id=first[b], **extra)[b, S]) == first[b]
        assert not (got[b, S:S + 4] == first[b]).any(), f"row {b} of {rows[b].numel()} tokens: an EOS before its own length reached {want}"
        _check_host_loop(tap, rows, S, eos=first[b], min_len=want)


@pytest.mark.parametrize("name", CASES)
def test_bad_words_and_suppress_tokens(name):
    plain, _, rows, S = _generate(name)
    p0 = sorted({int(t) for t in plain[:, S]})
    one, tap1, _, _ = _generate(name, bad_words_ids=[[t] for t in p0])
    same, _, _, _ = _generate(name, suppress_tokens=p0)
    assert torch.equal(one, same), "suppress_tokens are one-token bad words"
    assert not any(int(t) in p0 for t in one[:, S:].reshape(-1))
    _check_host_loop(tap1, rows, S, words=[[t] for t in p0])
    # the two-token word: taken from the run under the one-token bans, not from the plain completion -- the plain completion starts with
    # a token that is banned here, so a word from it could never be completed and its ban would show nothing; this one would be produced
    pair = one[0, S:S + 2].tolist()
    words = [[t] for t in p0] + [pair]
    two, tap2, _, _ = _generate(name, bad_words_ids=words)
    _check_host_loop(tap2, rows, S, words=words)
    for b, prompt in enumerate(rows):
        whole = prompt.tolist() + two[b, S:].tolist()
        assert tuple(pair) not in _bigrams(whole)[len(prompt) - 1:], f"row {b}: the word {pair} was completed in {whole}"
    assert not torch.equal(two, one)


@pytest.mark.parametrize("name", CASES)
def test_sampler_never_draws_a_banned_token_and_repeats_under_a_seed(name):
    plain, _, rows, S = _generate(name)
    sup = sorted({int(t) for t in plain[:, S:].reshape(-1)})[:6]
    more = dict(do_sample=True, temperature=1.4, top_k=12, top_p=0.95, repetition_penalty=1.2, seed=7, no_repeat_ngram_size=2, suppress_tokens=sup)
    a, tap, _, _ = _generate(name, **more)
    b, _, _, _ = _generate(name, **more)
    assert torch.equal(a, b), "the same seed gave two outputs"
    _check_host_loop(tap, rows, S, n=2, words=[[t] for t in sup], argmax=False)
    assert not any(int(t) in sup for t in a[:, S:].reshape(-1))


def test_llama_multinomial_path_reads_the_processed_row():
    name = "llama_uniform"
    plain, _, rows, S = _generate(name)
    sup = sorted({int(t) for t in plain[:, S:].reshape(-1)})
    torch.manual_seed(3)
    got, tap, _, _ = _generate(name, do_sample=True, temperature=0.05, suppress_tokens=sup, no_repeat_ngram_size=2)
    _check_host_loop(tap, rows, S, n=2, words=[[t] for t in sup], argmax=False)
    assert not any(int(t) in sup for t in got[:, S:].reshape(-1))


@pytest.mark.parametrize("name", CASES)
def test_logprobs_stay_the_models_own(name):
    m, kw, rows = _cases()[name]
    S = kw["input_ids"].shape[1]
    tap = _Tap()
    ids, lps = m.generate(**kw, stopping_criteria=[tap], return_logprobs=True, no_repeat_ngram_size=2)
    assert lps.shape == (len(rows), ids.shape[1] - S) and bool(torch.isfinite(lps).all())
    ranks = []
    for t, (_, scores) in enumerate(tap.steps):
        dev = scores.cuda().contiguous()
        rank = torch.zeros((len(rows),), dtype=torch.int32, device="cuda")
        want = ops.token_logprob_rows(dev, ids[:, S + t].contiguous(), torch.zeros((len(rows),), dtype=torch.float32, device="cuda"), rank=rank)
        assert torch.equal(bits(want), bits(lps[:, t].contiguous())), f"step {t}: not the log-softmax of the raw logits"
        ranks += rank.cpu().tolist()
    assert max(ranks) > 0, "every token was the raw row's maximum: the constraint never bit"


def _inflight_examples(kind):
    if kind == "mpt":
        m = _mpt()
        g = torch.Generator().manual_seed(9)
        audio = [5, 93, 95, 95, 95, 95, 94]
        ex = []
        for i in range(7):
            body = ([11 + i, 23, 42] * 6)[: 6 + 2 * i]
            ex.append((torch.tensor(audio + body), torch.randn(4, 64, generator=g), [10, 3, 7, 10, 1, 9, 5][i]))
        return m, None, ex
    from llark_amd.m2t.infer_driver import build_prompt_ids
    tok = LG._tok()
    m = LG._tiny_model(tok, 4, 256)
    end_seq = tok("\n### Assistant:").input_ids[1:]
    rng = np.random.default_rng(31)
    ex = []
    for i in range(8):
        clip = i // 4
        if i % 4 == 0:
            frames = [70, 66][clip]
            enc = torch.from_numpy(rng.standard_normal((frames, LG.MM)).astype(np.float32))
        ex.append((build_prompt_ids(LG.PROMPTS[i % 4], frames, tok, LG.MM_CFG, end_seq, audio_first=True), enc, int(rng.integers(3, 11)), f"clip{clip}"))
    for j, (first, length) in enumerate(((2, 30), (4, 17), (12, 30), (14, 30))):       # text only: prompts after which the plain run repeats
        ex.insert(2 * j + 1, (_words_prompt(first, length), None, 8 + j, None))
    return m, tok, ex


@pytest.mark.parametrize("kind", ["llama", "mpt"])
def test_inflight_completions_do_not_depend_on_the_slot_count(kind):
    from llark_amd.m2t.constraints import TokenConstraints
    from llark_amd.m2t.infer_driver import generate_inflight
    m, tok, ex = _inflight_examples(kind)
    cons = TokenConstraints(no_repeat_ngram_size=2, min_new_tokens=2)

    def run(n, **kw):
        return dict(generate_inflight(m, iter(ex), slots=n, max_new_tokens=N, keywords=(), constraints=cons, **kw))
    one, three = run(1), run(3)
    plain = dict(generate_inflight(m, iter(ex), slots=3, max_new_tokens=N, keywords=()))
    assert sorted(one) == sorted(three) == list(range(len(ex)))
    for i, e in enumerate(ex):
        assert torch.equal(one[i], three[i]), f"example {i}: {one[i].tolist()} with 1 slot, {three[i].tolist()} with 3"
        whole, p = one[i].tolist(), e[0].numel()
        assert len(whole) <= p + e[2]                               # the example's own budget wins over min_new_tokens
        bg = _bigrams(whole)[p - 1:]
        assert not set(bg) & set(_bigrams(whole[:p])) and len(set(bg)) == len(bg), f"example {i}: a bigram repeats"
    assert any(not torch.equal(plain[i], three[i]) for i in plain)
    if kind == "llama":
        trace = []
        shared = run(3, share_prefix=True, trace=trace)
        assert any(e[0] == "fork" for e in trace), "no example was forked: the whole-prompt admit was not exercised"
        for i in range(len(ex)):
            assert torch.equal(shared[i], three[i]), f"example {i} under share_prefix: {shared[i].tolist()} vs {three[i].tolist()}"


def _add(tf, name, data):
    ti = tarfile.TarInfo(name)
    ti.size = len(data)
    tf.addfile(ti, io.BytesIO(data))


def test_shards_cli_round_trip(tmp_path, monkeypatch):
    """`python -m llark_amd.m2t.infer_driver shards ... --no-repeat-ngram-size 2 --min-new-tokens 3` on a two-example shard."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from llark_amd.m2t import infer_driver as D
    from llark_amd.m2t.constraints import TokenConstraints
    from llark_amd.m2t.llamav2 import WrappedLlamav2Config, WrappedLlamav2ForCausalLM
    from llark_amd.m2t.prompting import DEFAULT_CONVERSATION_HEADER
    words = sorted(set((DEFAULT_CONVERSATION_HEADER + " ### Human: Assistant: <empty> what is k0 ? it . tempo fast").split()))
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "\n": 3}
    for wd in words:
        vocab.setdefault(wd, len(vocab))
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    ckpt = tmp_path / "ckpt"
    PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", bos_token="<s>", eos_token="</s>").save_pretrained(str(ckpt))
    cfg = WrappedLlamav2Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                               vocab_size=len(vocab), max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.mm_hidden_size = 96
    torch.manual_seed(0)
    WrappedLlamav2ForCausalLM(cfg).save_pretrained(str(ckpt))
    buf = io.BytesIO()
    np.save(buf, np.random.default_rng(3).standard_normal((4, 96)).astype(np.float32))
    with tarfile.open(tmp_path / "s-000.tar", "w") as tf:
        resp = {"response": [{"question": "what is k0 ?", "answer": "it is k0 ."}, {"question": "tempo ?", "answer": "fast ."}]}
        _add(tf, "k0.json", json.dumps(resp).encode())
        _add(tf, "k0.audio_encoding.npy", buf.getvalue())
    args = ["--model_name_or_path", str(ckpt), "--eval_data_path", str(tmp_path / "s-000.tar"), "--max_new_tokens", "8", "--slots", "2",
            "--mm_hidden_size", "96", "--model_max_length", "128"]
    outs, real = [], D.generate_inflight

    def spy(model, examples, **kw):
        seen = kw.get("constraints")
        for item in real(model, examples, **kw):
            outs.append((seen, item[0], item[1]))
            yield item
    monkeypatch.setattr(D, "generate_inflight", spy)
    torch.manual_seed(1)                        # loading draws the embedding rows of the added tokens from torch's generator
    plain = D.main_shards(args + ["--outfile", str(tmp_path / "a.csv")])
    n_plain = len(outs)
    torch.manual_seed(1)
    recs = D.main_shards(args + ["--outfile", str(tmp_path / "b.csv"), "--no-repeat-ngram-size", "2", "--min-new-tokens", "3"])
    assert len(plain) == len(recs) == 2 and n_plain == 2 and len(outs) == 4
    assert all(o[0] is None for o in outs[:2]) and all(o[0] == TokenConstraints(no_repeat_ngram_size=2, min_new_tokens=3) for o in outs[2:])
    for a, b in zip(sorted(outs[:2], key=lambda o: o[1]), sorted(outs[2:], key=lambda o: o[1])):
        x, y = a[2].tolist(), b[2].tolist()                        # the same example: what the two runs share holds its prompt
        p = next((i for i in range(min(len(x), len(y))) if x[i] != y[i]), min(len(x), len(y)))
        bg = _bigrams(y)
        assert len(set(bg[p - 1:])) == len(bg[p - 1:]) and not set(bg[p - 1:]) & set(bg[:p - 1]), f"a bigram repeats in {y} past {p}"


def test_beams_with_a_bigram_ban_follow_the_reference():
    """generate(num_beams=3, no_repeat_ngram_size=2), two examples of different lengths: the trellis, the returned ids and the returned
    log-probabilities are those of the constrained BeamRef loop replayed on the logits each step saw."""
    tok, m = _llama()
    rows = _llama_rows()
    ids, mask = LG._padded(rows, True)
    B, NEW = 3, 9
    kw = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), max_new_tokens=NEW, num_beams=B, return_logprobs=True)
    free_ids, _ = m.generate(**kw, eos_token_id=-1, no_repeat_ngram_size=2)
    eos = int(free_ids[0, ids.shape[1] + 3])                       # an eos that the search will meet
    seen, held = [], {}

    def observer(beam, eng):
        held["beam"] = beam
        beam.observe_logits = lambda step, logits: seen.append(logits[:, : beam.vocab].cpu())
    m.beam_observer = observer
    try:
        got_ids, got_lps = m.generate(**kw, eos_token_id=eos, no_repeat_ngram_size=2, min_new_tokens=2)
    finally:
        m.beam_observer = None
    beam = held["beam"]
    assert beam.constraints is not None and not beam.constraints.full()
    ref = CR.ConstrainedBeamRef([r.tolist() for r in rows], B, beam.vocab, eos=eos, pad=beam.pad, n=2, min_new=2)
    for step, lg in enumerate(seen):
        x = lg.numpy()
        ref.step(x)
        parent, token, lp = ref.ref.trellis[-1]
        tr = beam.trellis[step].cpu().numpy()
        assert tr[:, 0].tolist() == parent.tolist() and tr[:, 1].tolist() == token.tolist(), f"step {step}: the device decided otherwise"
        got_lp = np.ascontiguousarray(tr[:, 2]).view(np.float32)
        for slot in range(len(parent)):
            if parent[slot] >= 0:
                assert abs(float(got_lp[slot]) - lp[slot]) <= R.tol_of(x[parent[slot]], int(token[slot])), f"step {step} slot {slot}"
    assert ref.ref.steps == beam.steps
    # the device's histories are the beams' own
    hl = beam.constraints.hist_len.cpu().tolist()
    live = [s for s in range(len(hl)) if not ref.ref.done[s // B]]
    for s in live:
        assert beam.constraints.hist[s, :hl[s]].cpu().tolist() == ref.hists[s]
    want_ids, want_lps = R.layout(ids.numpy(), ref.ref.finalize(1), eos, beam.pad, NEW)
    assert got_ids.cpu().tolist() == want_ids.tolist()
    g = got_lps.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want_lps)) and np.allclose(np.nan_to_num(g), np.nan_to_num(want_lps), rtol=0, atol=2e-5)
    S = ids.shape[1]
    for b, prompt in enumerate(rows):
        gen = [int(t) for t in got_ids[b, S:].tolist()]
        if eos in gen:                                             # generate puts an eos behind a short row, ended or not: left out here
            assert gen.index(eos) >= 2, "an EOS before min_new_tokens"
            gen = gen[:gen.index(eos)]
        whole = prompt.tolist() + gen
        bg = _bigrams(whole)[len(prompt) - 1:]
        assert not set(bg) & set(_bigrams(prompt.tolist())) and len(set(bg)) == len(bg), f"example {b}: a bigram repeats in {whole}"
    unconstrained, _ = m.generate(**kw, eos_token_id=eos)
    assert unconstrained.shape != got_ids.shape or not torch.equal(unconstrained, got_ids)
