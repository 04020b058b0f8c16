"""CPU: the arguments of guided choice -- what is refused and with which words, what collapses, and how the CLI and the in-flight
driver hand the sets on (llark_amd/m2t/guide.py, infer_driver.py)."""
import json

import pytest
import torch

from llark_amd.m2t.guide import ChoiceSets, DeviceGuide, choices_from_json, choices_from_strings, guide_from_generate, require_eos


@pytest.mark.parametrize("sets, words", [
    ([], "non-empty list of choice sets"),
    ([[]], "non-empty list of non-empty token-id sequences"),                 # an empty set
    ([[[1], []]], r"non-empty token-id sequences, got the sequence \[\]"),    # an empty sequence
    ([[[1, -2]]], "token id must be an integer in 0"),
    ([[[1, 2.5]]], "token id must be an integer in 0"),
    ([[[True]]], "token id must be an integer in 0"),
    ([["ab"]], "got the sequence 'ab'"),
])
def test_bad_sets_are_refused_by_name(sets, words):
    with pytest.raises(ValueError, match=words):
        ChoiceSets(sets)


def test_sets_are_frozen_sorted_and_without_duplicates():
    c = ChoiceSets([[[3, 4], [1], [3, 4], (1,)], [torch.tensor([7, 8])]])
    assert c.sets == (((1,), (3, 4)), ((7, 8),))
    with pytest.raises(Exception):
        c.sets = ()
    assert c == ChoiceSets([[[1], [3, 4]], [[7, 8]]])


def test_out_of_range_ids_are_refused_when_the_table_is_built():
    c = ChoiceSets([[[1, 2]], [[5, 99]]])
    with pytest.raises(ValueError, match=r"choice set 1: token id 99 outside \[0, vocab = 99\)"):
        c.table(99)
    off, tok, node, term, roots = c.table(100)
    assert roots == [0, 3] and tok.tolist() == [1, 2, 5, 99] and term.tolist() == [0, 0, 1, 0, 0, 1]


@pytest.mark.parametrize("eos", [None, -1, True, 2.0])
def test_a_missing_eos_is_refused_by_the_arguments_name(eos):
    with pytest.raises(ValueError, match="a choice set needs eos_token_id >= 0"):
        require_eos(eos)
    with pytest.raises(ValueError, match="a choice set needs eos_token_id >= 0"):
        DeviceGuide(ChoiceSets([[[1]]]), 2, 8, "cpu", eos)
    with pytest.raises(ValueError, match="generation_config.eos_token_id >= 0"):
        require_eos(eos, "generation_config.eos_token_id")


def test_an_eos_outside_the_vocabulary_is_refused():
    with pytest.raises(ValueError, match=r"eos_token_id = 8 outside \[0, vocab = 8\)"):
        DeviceGuide(ChoiceSets([[[1]]]), 2, 8, "cpu", 8)


def test_generate_argument_one_set_or_one_per_row():
    assert guide_from_generate(None, 3) == (None, None)
    g, idx = guide_from_generate([[4, 5], [6]], 3)                            # one set for every row
    assert g.sets == (((4, 5), (6,)),) and idx == [0, 0, 0]
    g, idx = guide_from_generate([[[4, 5]], None, [[6], [7]]], 3)             # one set, or None, per row
    assert g.sets == (((4, 5),), ((6,), (7,))) and idx == [0, None, 1]
    assert guide_from_generate([None, None], 2) == (None, None)
    with pytest.raises(ValueError, match="allowed_continuations: a per-row list needs one choice set .or None. per row: 3 rows, got 2 entries"):
        guide_from_generate([[[4]], None], 3)
    with pytest.raises(ValueError, match="allowed_continuations must be one choice set"):
        guide_from_generate([], 1)
    with pytest.raises(ValueError, match="allowed_continuations: a choice set must be a non-empty list"):
        guide_from_generate([[[4]], []], 2)
    with pytest.raises(ValueError, match="allowed_continuations: .*got the sequence \\[\\]"):
        guide_from_generate([[4], []], 2)


class _Tok:
    """Splits on characters: ' ab' -> [32, 97, 98]; special tokens would be a leading 1."""

    def __call__(self, text, add_special_tokens=True):
        ids = ([1] if add_special_tokens else []) + [ord(c) for c in text]
        return type("Enc", (), {"input_ids": ids})()


def test_choices_from_strings_tokenises_lead_plus_label_without_special_tokens():
    assert choices_from_strings(_Tok(), ["ab", "c"]) == [[32, 97, 98], [32, 99]]
    assert choices_from_strings(_Tok(), ["ab"], lead="") == [[97, 98]]
    for bad in ([], ["a", ""], "ab", [3]):
        with pytest.raises(ValueError, match="non-empty list of non-empty strings"):
            choices_from_strings(_Tok(), bad)


def test_choices_json_parsing():
    assert choices_from_json('["C major", "A minor"]') == ["C major", "A minor"]
    for bad in ('{"a": 1}', "[]", '["a", 3]', '["a", ""]', '"a"'):
        with pytest.raises(ValueError, match="--choices-json: a non-empty JSON list of non-empty strings"):
            choices_from_json(bad)
    with pytest.raises(ValueError, match="--choices-json: not JSON"):
        choices_from_json("[a,")


def test_shards_cli_choices_json_becomes_one_choice_set(monkeypatch, tmp_path):
    from llark_amd.m2t import infer_driver as D
    seen = []
    monkeypatch.setattr(D, "_load_for_inference", lambda args, n: ("model", _Tok(), [1], {}))
    monkeypatch.setattr(D, "infer_from_shards", lambda *a, **k: seen.append(k) or [])
    base = ["--model_name_or_path", "checkpoints/llama", "--eval_data_path", "x.tar"]
    f = tmp_path / "labels.json"
    f.write_text(json.dumps(["ab", "c"]))
    D.main_shards(base + ["--choices-json", str(f)])
    assert seen[-1]["choice_sets"] == [[[32, 97, 98], [32, 99]]]
    D.main_shards(base)
    assert "choice_sets" not in seen[-1]
    f.write_text('{"not": "a list"}')
    with pytest.raises(SystemExit):
        D.main_shards(base + ["--choices-json", str(f)])
    with pytest.raises(SystemExit):
        D.main_shards(base + ["--choices-json", str(tmp_path / "missing.json")])


class _Backend:
    def __init__(self):
        self.calls = []

    def prefill(self, slots, prompts, encodings, **kw):
        self.calls.append(kw)
        return [2] * len(slots)

    def decode(self):
        return []

    def release(self, slots):
        pass


class _ModelWithBackend:
    generation_config = type("GC", (), {"eos_token_id": 2})()

    def slot_backend(self, n):
        return _Backend()


def test_inflight_refuses_choice_sets_with_a_models_own_slot_backend_and_a_stray_index():
    from llark_amd.m2t.infer_driver import InflightScheduler, generate_inflight
    ex = [(torch.tensor([5, 6]), None, None, None, 0)]
    with pytest.raises(ValueError, match="choice_sets need the engine's own slot backend"):
        list(generate_inflight(_ModelWithBackend(), ex, slots=1, keywords=(), choice_sets=[[[1]]]))
    with pytest.raises(ValueError, match="choice_sets must be a non-empty list of choice sets"):
        list(generate_inflight(type("M", (), {"generation_config": None})(), ex, slots=1, keywords=(), choice_sets=[]))
    with pytest.raises(ValueError, match="example 0 names the choice set 0, but no choice_sets were given"):
        list(generate_inflight(_ModelWithBackend(), ex, slots=1, keywords=()))
    # the scheduler hands each prefill call the indices of its examples, None for an unconstrained one
    b = _Backend()
    exs = [(torch.tensor([5]), None, None, None, 1), (torch.tensor([6]), None), (torch.tensor([7]), None, None, None, None)]
    out = list(InflightScheduler(b, 2, eos=2, choices=True).run(exs))
    assert [o[1].tolist() for o in out] == [[5, 2], [6, 2], [7, 2]] and [c["choice"] for c in b.calls] == [[1, None], [None]]
    b = _Backend()
    list(InflightScheduler(b, 2, eos=2).run(exs[1:2]))
    assert b.calls == [{}]                                                    # off: the backend's signature is what it was


def test_engine_slots_need_the_models_eos_for_choice_sets():
    from llark_amd.m2t.infer_driver import EngineSlots

    class _Eng:
        device = "cpu"

        def init_slots(self, n):
            pass

    class _M:
        engine = _Eng()
        generation_config = type("GC", (), {"eos_token_id": None})()

        def get_model(self):
            return type("Inner", (), {"audio_encoder_config": object()})()
    with pytest.raises(ValueError, match="a choice set needs generation_config.eos_token_id >= 0"):
        EngineSlots(_M(), 2, choice_sets=ChoiceSets([[[1]]]))


def test_shards_need_choice_of_for_several_sets():
    from llark_amd.m2t.infer_driver import infer_from_shards
    with pytest.raises(ValueError, match="several choice_sets need choice_of"):
        infer_from_shards(None, None, "x.tar", {}, [1], choice_sets=[[[1]], [[2]]])
    with pytest.raises(ValueError, match="choice_of without choice_sets"):
        infer_from_shards(None, None, "x.tar", {}, [1], choice_of=lambda conv: 0)
