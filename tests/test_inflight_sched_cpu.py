"""In-flight slot scheduling without a GPU: the scheduler of generate_inflight against a fake model (slot assignment, refill order,
per-row keyword / EOS / budget stops, output order) and infer_from_shards (the record contract of the reference's
scripts/inference/infer_from_webdataset.py) on a synthetic tar shard."""
import io
import json
import os
import sys
import tarfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from toy_tokenizer import ToyTokenizer  # noqa: E402

EOS = 2


class FakeBackend:
    """Slot backend whose token after k generated tokens is script[prompt[0]][k] (then `filler`), checking the slot protocol."""

    def __init__(self, n, scripts, filler):
        self.n, self.scripts, self.filler = n, scripts, filler
        self.slots = [None] * n
        self.calls = []

    def _next(self, b):
        prompt, gen = self.slots[b]
        sc = self.scripts.get(int(prompt[0]), [])
        t = sc[len(gen)] if len(gen) < len(sc) else self.filler
        gen.append(t)
        return t

    def prefill(self, slots, prompts, encodings):
        self.calls.append(("prefill", list(slots)))
        out = []
        for b, p in zip(slots, prompts):
            assert self.slots[b] is None, f"slot {b} prefilled while busy"
            self.slots[b] = (p.tolist(), [])
            out.append(self._next(b))
        return out

    def decode(self):
        assert any(s is not None for s in self.slots), "decode step with every slot free"
        self.calls.append(("decode",))
        return [self._next(b) if self.slots[b] is not None else -1 for b in range(self.n)]

    def release(self, slots):
        for b in slots:
            assert self.slots[b] is not None
            self.slots[b] = None


class FakeModel:
    def __init__(self, scripts, filler):
        self.scripts, self.filler = scripts, filler
        self.generation_config = type("GC", (), {"eos_token_id": EOS})()
        self.backends = []

    def slot_backend(self, n):
        be = FakeBackend(n, self.scripts, self.filler)
        self.backends.append(be)
        return be


def _tok():
    tok = ToyTokenizer()
    for w in "a b c ### stop x y".split():
        tok.encode(w)
    return tok


def _solo(prompt, script, filler, budget, tok):
    """What generate_batch / the per-example generate loop return for one example under the same stopping rules."""
    from llark_amd.m2t.generate import KeywordsStoppingCriteria
    stop = KeywordsStoppingCriteria(["###"], tok, prompt[None])
    out = prompt.tolist()
    for k in range(budget):
        t = script[k] if k < len(script) else filler
        out.append(t)
        if t == EOS or stop(torch.tensor([out]), None):
            break
    return out


def test_scheduler_slots_refill_stops_and_order():
    from llark_amd.m2t.infer_driver import generate_inflight
    tok = _tok()
    a, b, c, kw, x = (tok.vocab[w] for w in ("a", "b", "c", "###", "x"))
    # example i has prompt [100 + i, ...] and the token script below; budgets in the third field
    scripts = {100: [a, b, c, a, b],            # budget 3
               101: [EOS],                      # EOS right after the prompt: its slot is refilled before any decode step
               102: [a, kw, b],                 # keyword on the 2nd token
               103: [b, b, b, b, b, b],         # runs to the default budget (6)
               104: [c, EOS, a],                # EOS on the 2nd token
               105: [a],                        # budget 1
               106: [x, x, kw]}                 # keyword on the 3rd token
    budgets = {100: 3, 105: 1}
    examples = [(torch.tensor([100 + i] + [a] * (i + 1)), None, budgets.get(100 + i)) for i in range(7)]
    m = FakeModel(scripts, filler=x)
    trace = []
    got = list(generate_inflight(m, iter(examples), slots=2, max_new_tokens=6, tokenizer=tok, trace=trace))
    be = m.backends[0]
    assert be.slots == [None, None]                                       # every slot released at the end
    # each example's ids are its solo run
    for idx, ids in got:
        p = examples[idx][0]
        want = _solo(p, scripts[int(p[0])], x, budgets.get(int(p[0]), 6), tok)
        assert ids.tolist() == want, f"example {idx}"
    assert sorted(i for i, _ in got) == list(range(7))
    # yield order = completion order; rows finishing in the same step in input order
    assert [i for i, _ in got] == [e[2] for e in trace if e[0] == "done"]
    # slot assignment and refill order: free slots ascending, examples in input order
    prefills = [e for e in trace if e[0] == "prefill"]
    assert prefills[0] == ("prefill", (0, 1), (0, 1))
    assert trace[1] == ("done", 1, 1) and trace[2] == ("prefill", (1,), (2,))    # EOS at once -> refilled before decoding
    assert [i for e in prefills for i in e[2]] == list(range(7))
    assert be.calls[:3] == [("prefill", [0, 1]), ("prefill", [1]), ("decode",)]
    # example 0 (budget 3) leaves slot 0 after two decode steps; example 2 (keyword on its 2nd token) leaves slot 1 at the first
    done0 = trace.index(("done", 0, 0))
    assert ("done", 1, 2) in trace[:done0 + 1]
    # with one slot: the same results, strictly in input order
    m1 = FakeModel(scripts, filler=x)
    one = list(generate_inflight(m1, iter(examples), slots=1, max_new_tokens=6, tokenizer=tok))
    assert [i for i, _ in one] == list(range(7))
    assert {i: t.tolist() for i, t in one} == {i: t.tolist() for i, t in got}


def test_scheduler_needs_tokenizer_for_keywords_and_slots():
    from llark_amd.m2t.infer_driver import InflightScheduler, generate_inflight
    with pytest.raises(ValueError, match="tokenizer"):
        list(generate_inflight(FakeModel({}, 5), iter([]), slots=2))
    with pytest.raises(ValueError):
        InflightScheduler(FakeBackend(1, {}, 5), 0)
    # no keywords: EOS and budgets only; an empty input yields nothing and never decodes
    m = FakeModel({7: [5, 5, EOS]}, 5)
    assert [t.tolist() for _, t in generate_inflight(m, iter([(torch.tensor([7]), None)]), slots=3, max_new_tokens=10, keywords=())] == \
        [[7, 5, 5, EOS]]
    m2 = FakeModel({}, 5)
    assert list(generate_inflight(m2, iter([]), slots=3, keywords=())) == [] and m2.backends[0].calls == []


def _add(tf, name, data):
    info = tarfile.TarInfo(name)
    info.size = len(data)
    tf.addfile(info, io.BytesIO(data))


def _npy(a):
    buf = io.BytesIO()
    np.save(buf, a)
    return buf.getvalue()


def _make_shard(path, keys, frames=3, rng=None):
    """Like tests/test_data_cpu.py::_make_shard: two (question, answer) pairs per sample, .npy encodings."""
    rng = rng or np.random.default_rng(0)
    with tarfile.open(path, "w") as tf:
        for k in keys:
            enc = rng.standard_normal((frames, 8)).astype(np.float32)
            resp = {"response": [{"question": f"what is {k} ?", "answer": f"it is {k} ."}, {"question": "tempo ?", "answer": "fast ."}]}
            _add(tf, f"{k}.json", json.dumps(resp).encode())
            _add(tf, f"{k}.audio_encoding.npy", _npy(enc))


class RecordingModel(FakeModel):
    """Answers "y y ###" to every prompt and keeps the prompts it was given."""

    def __init__(self, tok):
        y, kw = tok.vocab["y"], tok.vocab["###"]
        super().__init__({}, filler=y)
        self.kw, self.prompts = kw, []

    def slot_backend(self, n):
        be = super().slot_backend(n)
        outer = self
        orig = be.prefill

        def prefill(slots, prompts, encodings):
            outer.prompts += [p.tolist() for p in prompts]
            for p, e in zip(prompts, encodings):
                assert e is not None and e.shape == (3, 8)
                be.scripts[int(p[0])] = [outer.filler, outer.filler, outer.kw]
            return orig(slots, prompts, encodings)

        be.prefill = prefill
        return be


def test_infer_from_shards_records(tmp_path):
    import pandas as pd
    from llark_amd.m2t import infer_driver as D
    tok = ToyTokenizer()
    tok.add_tokens(["<audio_patch>", "<audio_start>", "<audio_end>"], special_tokens=True)
    for w in "y ### Describe this .".split():
        tok.encode(w)
    end_seq = tok("\n### Assistant:").input_ids[1:]
    mm = dict(is_multimodal=True, sep_audio_conv_front=False, use_audio_start_end=True)
    _make_shard(tmp_path / "s-000.tar", ["k0", "k1"])
    _make_shard(tmp_path / "s-001.tar", ["k2"])
    shards = str(tmp_path / "s-{000..001}.tar")
    out = tmp_path / "res" / "out.csv"
    m = RecordingModel(tok)
    recs = D.infer_from_shards(m, tok, shards, mm, end_seq, outfile=str(out), slots=3, max_new_tokens=8, seed=0)
    df = pd.read_csv(out, keep_default_na=False)
    assert list(df.columns) == ["example_id", "prompt_text", "original_completion_text", "model_completion_text"]
    assert list(df["example_id"]) == ["k0", "k0", "k1", "k1", "k2", "k2"]                 # tar key, repeated per question, input order
    answers = ["it is k0 .", "fast .", "it is k1 .", "fast .", "it is k2 .", "fast ."]
    questions = ["what is k0 ?", "tempo ?", "what is k1 ?", "tempo ?", "what is k2 ?", "tempo ?"]
    for r, ans, q in zip(recs, answers, questions):
        assert r["original_completion_text"].split(" \n")[0].strip() == ans, r
        assert q in r["prompt_text"] and "Assistant:" in r["prompt_text"] and ans not in r["prompt_text"]
        assert r["model_completion_text"] == "y y ###"
    assert len(m.prompts) == 6 and all(tok.vocab["<audio_start>"] in p for p in m.prompts)
    # --prompt overrides every question (audio first); the original completion stays the pair's answer; max_samples caps examples
    m2 = RecordingModel(tok)
    recs2 = D.infer_from_shards(m2, tok, shards, mm, end_seq, slots=2, max_new_tokens=8, prompt="Describe this .", max_samples=4)
    assert [r["example_id"] for r in recs2] == ["k0", "k0", "k1", "k1"]
    assert all(r["prompt_text"] == "Describe this ." for r in recs2)
    assert [r["original_completion_text"].split(" \n")[0].strip() for r in recs2] == answers[:4]
    for p in m2.prompts:
        txt = tok.decode(p)
        assert "Describe this ." in txt and "what is" not in txt and "tempo" not in txt
        assert txt.index("<audio_start>") < txt.index("Describe")                      # audio first
