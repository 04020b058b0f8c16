"""CPU: the inference driver picks the backbone by name (the "mpt" rule of train.backbone_of), refuses --share-prefix for an MPT model
before anything loads, and EngineSlots asks the splice plan for the MPT wrapper's patch-token branch.  No weights, no GPU."""
from types import SimpleNamespace

import pytest
import torch


class _StubModel:
    """what _load_for_inference touches after from_pretrained"""

    def __init__(self, kind):
        self.kind = kind
        self.config = SimpleNamespace(mm_hidden_size=None)
        self.inner = SimpleNamespace(mm_projector=object(), audio_encoder_config=SimpleNamespace())
        self.calls = []

    def get_model(self):
        return self.inner

    def get_input_embeddings(self):
        return SimpleNamespace(weight=torch.zeros(8, 2))

    def resize_token_embeddings(self, n):
        self.calls.append(("resize", n))

    def initialize_audio_tokenizer(self, **kw):
        self.calls.append(("audio_tokenizer", kw["mm_use_audio_start_end"]))

    def cuda(self):
        return self

    def eval(self):
        return self

    def configure_engine(self, **kw):
        self.calls.append(("engine", kw))


class _StubTok:
    pad_token = "[PAD]"

    def get_vocab(self):
        return {"a": 0}

    def __call__(self, texts, add_special_tokens=False):
        return SimpleNamespace(input_ids=[[7, 8, 9]])


@pytest.mark.parametrize("name,want", [("checkpoints/mpt-1b-redpajama-200b", "mpt"), ("out/my-mpt-run/checkpoint-3", "mpt"),
                                       ("meta-llama/Llama-2-7b-chat-hf", "llama"), ("checkpoints/llark", "llama")])
def test_load_for_inference_picks_the_wrapper_by_name(monkeypatch, name, want):
    from llark_amd.m2t import infer_driver as D
    from llark_amd.m2t.llamav2 import WrappedLlamav2ForCausalLM
    from llark_amd.m2t.mpt import WrappedMPTForCausalLM
    seen = []

    def loader(kind):
        def from_pretrained(path, **kw):
            seen.append((kind, path, kw))
            return _StubModel(kind)
        return from_pretrained

    monkeypatch.setattr(WrappedMPTForCausalLM, "from_pretrained", staticmethod(loader("mpt")))
    monkeypatch.setattr(WrappedLlamav2ForCausalLM, "from_pretrained", staticmethod(loader("llama")))
    monkeypatch.setattr(D, "_load_tokenizer", lambda args: _StubTok())
    args = SimpleNamespace(model_name_or_path=name, model_max_length=256, mm_hidden_size=512, llm_precision="split")
    model, tok, end_seq, mm_cfg = D._load_for_inference(args, 5)
    assert [k for k, _, _ in seen] == [want] and seen[0][1] == name and model.kind == want
    assert seen[0][2]["torch_dtype"] == torch.bfloat16
    if want == "mpt":
        assert seen[0][2]["mm_hidden_size"] == 512                       # as train.main opens an MPT folder
    assert ("engine", dict(max_batch=5, max_seq=256, precision="split")) in model.calls and ("audio_tokenizer", True) in model.calls
    assert mm_cfg["use_audio_start_end"] and isinstance(tok, _StubTok)


def test_shards_share_prefix_is_refused_by_name_for_an_mpt_model(monkeypatch, capsys):
    from llark_amd.m2t import infer_driver as D

    def boom(*a, **k):
        raise AssertionError("the model must not be loaded")

    monkeypatch.setattr(D, "_load_for_inference", boom)
    with pytest.raises(SystemExit) as e:
        D.main_shards(["--model_name_or_path", "checkpoints/mpt-1b", "--eval_data_path", "x.tar", "--share-prefix"])
    assert e.value.code == 2 and "--share-prefix" in capsys.readouterr().err
    with pytest.raises(AssertionError, match="must not be loaded"):      # a Llama name goes on to load
        D.main_shards(["--model_name_or_path", "checkpoints/llama", "--eval_data_path", "x.tar", "--share-prefix"])
    with pytest.raises(SystemExit):
        D.main_shards(["--model_name_or_path", "checkpoints/mpt-1b", "--eval_data_path", "x.tar", "--slots", "65"])


class _StubEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.inits = []

    def init_slots(self, n, **kw):
        self.inits.append((n, kw))

    def prefill_slots(self, rows, segs, slots):
        self.segs = segs
        return torch.zeros(len(rows), 4)


@pytest.mark.parametrize("mpt", [True, False], ids=["mpt", "llama"])
def test_engine_slots_asks_for_the_patch_branch_on_an_mpt_model(monkeypatch, mpt):
    from llark_amd.m2t import infer_driver as D
    from llark_amd.m2t import llamav2
    from llark_amd.m2t.mpt import WrappedMPTForCausalLM
    assert WrappedMPTForCausalLM.audio_patch_branch is True
    calls = []

    def plan(ids, feats, cfg, has_past, **kw):
        calls.append(kw)
        return [(0, 1, feats[0])]

    monkeypatch.setattr(llamav2, "plan_audio_splice", plan)
    model = SimpleNamespace(engine=_StubEngine(), get_model=lambda: SimpleNamespace(audio_encoder_config=SimpleNamespace(audio_patch_token=5)))
    if mpt:
        model.audio_patch_branch = True
    slots = D.EngineSlots(model, 3)
    assert model.engine.inits == [(3, {})]
    first = slots.prefill([2, 0], [torch.arange(6), torch.arange(4)], [torch.zeros(2, 8), None])
    assert first == [0, 0] and calls == [dict(patch_branch=True) if mpt else {}]
    assert [s[0] for s in model.engine.segs] == [0]
