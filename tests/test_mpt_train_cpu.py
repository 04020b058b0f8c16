"""CPU: how the training entry point picks the MPT backbone (the reference's rule, m2t/train.py:62) and which of its flags the MPT
training step refuses by name before any model is loaded."""
import pytest


def test_backbone_rule_on_the_reference_scripts_model_names():
    from llark_amd.m2t import train as T
    assert T.backbone_of("mosaicml/mpt-1b-redpajama-200b-dolly") == "mpt"            # scripts/training/train_mpt_model.sh
    assert T.backbone_of("meta-llama/Llama-2-7b-chat-hf") == "llama"                 # scripts/training/train_llark.sh
    assert T.backbone_of("checkpoints/mosaicml/mpt-1b-redpajama-200b-dolly/1234") == "mpt"      # the MPT script's --output_dir, reopened
    assert T.backbone_of("/data/ckpt") == "llama"


@pytest.mark.parametrize("flag", ["freeze_backbone", "lora_enable", "gradient_checkpointing"])
def test_mpt_name_refuses_the_flags_its_step_does_not_implement(flag):
    from llark_amd.m2t import train as T
    base = ["--train_data_path", "d", "--output_dir", "o", "--lora_dropout", "0.0"]
    mpt = T.build_arg_parser().parse_args(base + ["--model_name_or_path", "mosaicml/mpt-1b-redpajama-200b-dolly", f"--{flag}", "True"])
    with pytest.raises(NotImplementedError, match=f"--{flag}"):
        T.check_supported_recipe(mpt)
    # the same flag on a Llama name is a recipe the loop runs, and an MPT name without it passes
    T.check_supported_recipe(T.build_arg_parser().parse_args(base + ["--model_name_or_path", "meta-llama/Llama-2-7b-chat-hf", f"--{flag}", "True"]))
    T.check_supported_recipe(T.build_arg_parser().parse_args(base + ["--model_name_or_path", "mosaicml/mpt-1b-redpajama-200b-dolly"]))
    assert T.build_arg_parser().parse_args(base + ["--model_name_or_path", "mpt", "--pack_sequences", "True", "--fuse_accumulation", "True"]).pack_sequences


def test_mpt_wrapper_folder_round_trip(tmp_path):
    """``save_pretrained`` / ``from_pretrained`` of the wrapper: the folder format the CLI reads and the checkpoints are written in."""
    import torch
    from llark_amd.m2t.mpt import WrappedMPTConfig, WrappedMPTForCausalLM
    cfg = WrappedMPTConfig(d_model=256, n_heads=2, n_layers=1, expansion_ratio=2, max_seq_len=64, vocab_size=40, mm_hidden_size=32,
                           attn_config=dict(qk_ln=True, clip_qkv=3.0), no_bias=False, logit_scale=0.5)
    torch.manual_seed(0)
    m = WrappedMPTForCausalLM(cfg)
    m.save_pretrained(str(tmp_path / "mpt"))
    back = WrappedMPTForCausalLM.from_pretrained(str(tmp_path / "mpt"))
    assert back.config.to_dict() == m.config.to_dict()
    want, got = m.state_dict(), back.state_dict()
    assert set(want) == set(got) and all(torch.equal(want[k], got[k]) for k in want)
    wide = WrappedMPTForCausalLM.from_pretrained(str(tmp_path / "mpt"), torch_dtype=torch.bfloat16, mm_hidden_size=96)
    assert wide.transformer.mm_projector.weight.shape == (256, 96) and wide.transformer.wte.weight.dtype == torch.bfloat16
    sd = torch.load(tmp_path / "mpt" / "pytorch_model.bin")
    sd["transformer.blocks.0.attn.rotary.weight"] = torch.zeros(1)
    torch.save(sd, tmp_path / "mpt" / "pytorch_model.bin")
    with pytest.raises(KeyError, match="unexpected"):
        WrappedMPTForCausalLM.from_pretrained(str(tmp_path / "mpt"))
