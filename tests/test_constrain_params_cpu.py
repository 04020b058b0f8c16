"""Constrained decoding without a GPU: validation of TokenConstraints, refusals by name, and how the arguments travel -- from the two
command lines to infer_from_shards / infer_from_encodings, and from there to generate -- with nothing new passed on when nothing is asked."""
import pytest
import torch

from llark_amd.m2t.constraints import TokenConstraints, constraints_from_generate


@pytest.mark.parametrize("kw, name", [
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=65), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=2.0), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"),
    (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens="3"), "min_new_tokens"),
    (dict(min_length=-2), "min_length"), (dict(min_length=1.5), "min_length"),
    (dict(bad_words_ids=[[]]), "bad_words_ids"), (dict(bad_words_ids=[3]), "bad_words_ids"), (dict(bad_words_ids=[[1, -1]]), "bad_words_ids"),
    (dict(bad_words_ids="ab"), "bad_words_ids"), (dict(bad_words_ids=[[1.0]]), "bad_words_ids"),
    (dict(suppress_tokens=[-1]), "suppress_tokens"), (dict(suppress_tokens=5), "suppress_tokens"), (dict(suppress_tokens=[[1]]), "suppress_tokens"),
])
def test_bad_values_are_refused_by_name(kw, name):
    with pytest.raises(ValueError, match=name):
        TokenConstraints(**kw)
    with pytest.raises(ValueError, match=name):
        constraints_from_generate(**kw)


def test_table_caps_are_refused_by_name():
    from llark_amd import ops
    with pytest.raises(ValueError, match="bad_words_ids"):
        TokenConstraints(bad_words_ids=[[1]] * (ops.CONSTRAIN_MAX_WORDS + 1))
    with pytest.raises(ValueError, match="suppress_tokens"):
        TokenConstraints(bad_words_ids=[[1]] * ops.CONSTRAIN_MAX_WORDS, suppress_tokens=[2])


def test_active_and_normalisation():
    assert not TokenConstraints().active
    assert not TokenConstraints(None, None, None, None, None).active
    assert not TokenConstraints(0, [], (), 0, 0).active
    assert constraints_from_generate() is None and constraints_from_generate(0, [], [], 0, 0) is None
    for kw in (dict(no_repeat_ngram_size=1), dict(bad_words_ids=[[4, 5]]), dict(suppress_tokens=[7]), dict(min_new_tokens=1), dict(min_length=1)):
        assert TokenConstraints(**kw).active and constraints_from_generate(**kw) == TokenConstraints(**kw)
    c = TokenConstraints(3, [[1, 2], [3]], [9, 3], 4, 5)
    assert c.bad_words_ids == ((1, 2), (3,)) and c.suppress_tokens == (9, 3)
    assert c.words(eos=3) == ((1, 2), (9,)) and c.words(eos=None) == ((1, 2), (3,), (9,), (3,)) and c.words(eos=-1) == c.words()
    with pytest.raises(Exception):
        c.min_length = 1                                            # frozen


class _Backend:
    def prefill(self, slots, prompts, encodings):
        return [2] * len(slots)

    def decode(self):
        return []

    def release(self, slots):
        pass


class _ModelWithBackend:
    generation_config = type("GC", (), {"eos_token_id": 2})()

    def slot_backend(self, n):
        return _Backend()


@pytest.mark.parametrize("kw", [dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[1]]), dict(suppress_tokens=[1]), dict(min_new_tokens=2),
                                dict(min_length=2)])
def test_every_keyword_is_refused_with_a_models_own_slot_backend(kw):
    from llark_amd.m2t.infer_driver import generate_inflight
    ex = [(torch.tensor([5, 6]), None)]
    with pytest.raises(ValueError, match="constraints need the engine's own slot backend"):
        list(generate_inflight(_ModelWithBackend(), ex, slots=1, keywords=(), constraints=TokenConstraints(**kw)))
    # nothing asked: the model's backend serves the call as before
    for off in (None, TokenConstraints()):
        out = list(generate_inflight(_ModelWithBackend(), ex, slots=1, keywords=(), constraints=off))
        assert [o[1].tolist() for o in out] == [[5, 6, 2]]


def test_shards_cli_flags_become_token_constraints(monkeypatch):
    from llark_amd.m2t import infer_driver as D
    seen = []
    monkeypatch.setattr(D, "_load_for_inference", lambda args, n: ("model", "tok", [1], {}))
    monkeypatch.setattr(D, "infer_from_shards", lambda *a, **k: seen.append(k) or [])
    base = ["--model_name_or_path", "checkpoints/llama", "--eval_data_path", "x.tar"]
    D.main_shards(base + ["--no-repeat-ngram-size", "3", "--min-new-tokens", "8"])
    assert seen[-1]["constraints"] == TokenConstraints(no_repeat_ngram_size=3, min_new_tokens=8)
    D.main_shards(base + ["--min-new-tokens", "2"])
    assert seen[-1]["constraints"] == TokenConstraints(min_new_tokens=2)
    D.main_shards(base)
    assert "constraints" not in seen[-1]
    D.main_shards(base + ["--no-repeat-ngram-size", "0", "--min-new-tokens", "0"])
    assert "constraints" not in seen[-1]
    with pytest.raises(SystemExit):
        D.main_shards(base + ["--no-repeat-ngram-size", "65"])
    with pytest.raises(SystemExit):
        D.main_shards(base + ["--min-new-tokens", "-1"])


def test_encodings_cli_flags_reach_infer_from_encodings(monkeypatch):
    from llark_amd.m2t import infer_driver as D
    seen = []
    monkeypatch.setattr(D, "_load_for_inference", lambda args, n: ("model", "tok", [1], {}))
    monkeypatch.setattr(D, "infer_from_encodings", lambda *a, **k: seen.append(k) or [])
    base = ["--model_name_or_path", "checkpoints/llama", "--audio-encodings-dir", "reps", "--prompt", "p"]
    D.main(base + ["--no_repeat_ngram_size", "3", "--min_new_tokens", "4", "--num_beams", "4"])
    assert seen[-1]["no_repeat_ngram_size"] == 3 and seen[-1]["min_new_tokens"] == 4 and seen[-1]["num_beams"] == 4
    D.main(base)
    assert "no_repeat_ngram_size" not in seen[-1] and "min_new_tokens" not in seen[-1]
    with pytest.raises(SystemExit):
        D.main(base + ["--no_repeat_ngram_size", "-3"])


class _Recorder:
    """model.generate that records its keyword arguments and stops every row at once with the EOS."""
    generation_config = type("GC", (), {"eos_token_id": 2})()
    _engine = engine = type("Eng", (), {"device": torch.device("cpu")})()

    def __init__(self):
        self.calls = []

    def generate(self, input_ids=None, **kw):
        self.calls.append(kw)
        eos = torch.full((input_ids.shape[0], 1), 2, dtype=torch.int64)
        out = torch.cat((input_ids.cpu(), eos), dim=1)
        for c in kw.get("stopping_criteria") or []:
            c(out, None)
        return out


def test_generate_batch_and_beam_pass_the_arguments_on(monkeypatch):
    from llark_amd.m2t import infer_driver as D

    class _Never:
        def __init__(self, **kw):
            pass

        def __call__(self, ids, scores, **kw):
            return False
    monkeypatch.setattr(D, "KeywordsStoppingCriteria", _Never)
    ids = torch.tensor([[5, 6, 7]])
    enc = torch.zeros((1, 2, 4))
    m = _Recorder()
    D.generate_batch(m, ids, enc, None, 4)
    assert m.calls[-1]["eos_token_id"] == -1 and not {"no_repeat_ngram_size", "min_new_tokens"} & set(m.calls[-1])
    D.generate_batch(m, ids, enc, None, 4, no_repeat_ngram_size=3)
    assert m.calls[-1]["eos_token_id"] == -1 and m.calls[-1]["no_repeat_ngram_size"] == 3
    D.generate_batch(m, ids, enc, None, 4, min_new_tokens=2)                   # the ban on the EOS needs generate to know the EOS
    assert m.calls[-1]["eos_token_id"] == 2 and m.calls[-1]["min_new_tokens"] == 2
    D.generate_beam(m, ids, enc, None, 4, 3, 1.0, no_repeat_ngram_size=3, min_new_tokens=2)
    assert m.calls[-1]["num_beams"] == 3 and m.calls[-1]["no_repeat_ngram_size"] == 3 and m.calls[-1]["min_new_tokens"] == 2
    D.generate_beam(m, ids, enc, None, 4, 3, 1.0)
    assert not {"no_repeat_ngram_size", "min_new_tokens"} & set(m.calls[-1])
