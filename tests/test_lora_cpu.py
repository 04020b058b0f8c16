"""CPU: the host side of the LoRA recipe (llark_amd/m2t/lora.py, the flag checks of llark_amd/m2t/train.py) and the 2-rank
all-reduce over the small gradient table of a frozen-base trainer."""
import argparse
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_peft_key_mapping_round_trip():
    from llark_amd.m2t import lora as LO
    assert LO.peft_key(3, "q_proj", "A") == "base_model.model.model.layers.3.self_attn.q_proj.lora_A.weight"
    assert LO.peft_key(0, "down_proj", "B") == "base_model.model.model.layers.0.mlp.down_proj.lora_B.weight"
    for i in (0, 31):
        for mod in LO.TARGET_MODULES:
            for ab in "AB":
                assert LO.parse_peft_key(LO.peft_key(i, mod, ab)) == (i, mod, ab)
    assert LO.parse_peft_key("base_model.model.model.layers.0.mlp.q_proj.lora_A.weight") is None      # q_proj is not under mlp
    assert LO.parse_peft_key("model.layers.0.self_attn.q_proj.weight") is None
    assert LO.hf_weight_key(2, "up_proj") == "model.layers.2.mlp.up_proj.weight"
    cfg = LO.LoraConfig(r=8)
    ad = LO.init_adapters(cfg, 64, 96, 2, seed=0)
    assert set(ad) == {LO.peft_key(i, m, ab) for i in range(2) for m in LO.TARGET_MODULES for ab in "AB"}
    a, b = ad[LO.peft_key(1, "gate_proj", "A")], ad[LO.peft_key(1, "gate_proj", "B")]
    assert a.shape == (8, 64) and b.shape == (96, 8) and b.abs().max().item() == 0.0
    assert 0.5 / 8 < a.abs().max().item() <= 1.0 / 8                        # Kaiming-uniform, a = sqrt(5): bound 1 / sqrt(K)
    again = LO.init_adapters(cfg, 64, 96, 2, seed=0)
    assert all(torch.equal(ad[k], again[k]) for k in ad)                    # seeded
    assert not torch.equal(a, LO.init_adapters(cfg, 64, 96, 2, seed=1)[LO.peft_key(1, "gate_proj", "A")])
    sub = LO.init_adapters(LO.LoraConfig(r=8, target_modules=("q_proj", "v_proj")), 64, 96, 1)
    assert len(sub) == 4
    assert LO.LoraConfig.from_peft_dict(cfg.to_peft_dict()) == cfg


@pytest.mark.parametrize("r,rp", [(8, 64), (64, 64), (72, 128), (256, 256)])
def test_rank_padding(r, rp):
    from llark_amd.m2t import lora as LO
    assert LO.padded_rank(r) == rp and LO.LoraConfig(r=r).rp == rp
    g = torch.Generator().manual_seed(r)
    a, b = torch.randn(r, 40, generator=g), torch.randn(24, r, generator=g)
    at, bk = LO.a_to_kernel(a, rp), LO.b_to_kernel(b, rp)
    assert at.shape == (40, rp) and bk.shape == (24, rp) and at.dtype == bk.dtype == torch.float32
    assert torch.equal(at[:, :r], a.t()) and torch.equal(bk[:, :r], b)
    assert at[:, r:].abs().sum().item() == 0.0 and bk[:, r:].abs().sum().item() == 0.0
    assert torch.equal(LO.a_from_kernel(at, r), a) and torch.equal(LO.b_from_kernel(bk, r), b)


def test_merge_into_state_dict_against_float64():
    from llark_amd.m2t import lora as LO
    H, I = 32, 48
    cfg = LO.LoraConfig(r=8, alpha=4, target_modules=("q_proj", "down_proj"))
    g = torch.Generator().manual_seed(0)
    sd = {"model.layers.0.self_attn.q_proj.weight": torch.randn(H, H, generator=g).bfloat16(),
          "model.layers.0.self_attn.k_proj.weight": torch.randn(H, H, generator=g).bfloat16(),
          "model.layers.0.mlp.down_proj.weight": torch.randn(H, I, generator=g).bfloat16()}
    ad = {LO.peft_key(0, "q_proj", "A"): torch.randn(8, H, generator=g), LO.peft_key(0, "q_proj", "B"): torch.randn(H, 8, generator=g),
          LO.peft_key(0, "down_proj", "A"): torch.randn(8, I, generator=g), LO.peft_key(0, "down_proj", "B"): torch.randn(H, 8, generator=g)}
    out = LO.merge_into_state_dict(sd, ad, cfg)
    assert out is not sd and torch.equal(out["model.layers.0.self_attn.k_proj.weight"], sd["model.layers.0.self_attn.k_proj.weight"])
    for mod, par in (("q_proj", "self_attn"), ("down_proj", "mlp")):
        wk = f"model.layers.0.{par}.{mod}.weight"
        ref = sd[wk].double() + 0.5 * (ad[LO.peft_key(0, mod, "B")].double() @ ad[LO.peft_key(0, mod, "A")].double())
        assert out[wk].dtype == torch.bfloat16
        assert (out[wk].double() - ref).abs().max().item() <= 2.0 ** -8 * ref.abs().max().item()       # one bf16 rounding of the sum
        assert not torch.equal(out[wk], sd[wk])
    with pytest.raises(KeyError):
        LO.merge_into_state_dict(sd, {"model.layers.0.self_attn.q_proj.weight": torch.zeros(1)}, cfg)
    with pytest.raises(ValueError):
        LO.merge_into_state_dict(sd, ad, LO.LoraConfig(r=16, alpha=4))


def test_adapter_folder_round_trip(tmp_path):
    from llark_amd.m2t import lora as LO
    cfg = LO.LoraConfig(r=16, alpha=32, target_modules=("q_proj", "o_proj"))
    ad = LO.init_adapters(cfg, 64, 96, 2, seed=2)
    LO.save_adapter(str(tmp_path), ad, cfg)
    got, cfg2 = LO.load_adapter(str(tmp_path))
    assert cfg2 == cfg and set(got) == set(ad) and all(torch.equal(got[k], ad[k]) for k in ad)


def _args(**kw):
    base = dict(freeze_backbone=False, tune_mm_mlp_adapter=True, lr_scheduler_type="cosine", bf16=True, lora_enable=False, lora_r=64,
                lora_alpha=16.0, lora_dropout=0.0, lora_bias="none")
    base.update(kw)
    return argparse.Namespace(**base)


def test_check_supported_recipe():
    from llark_amd.m2t.lora import LoraConfig
    from llark_amd.m2t.train import check_supported_recipe, lora_config_of
    check_supported_recipe(_args())
    check_supported_recipe(_args(freeze_backbone=True))
    check_supported_recipe(_args(lora_enable=True, lora_r=8, lora_alpha=16.0))
    check_supported_recipe(_args(lora_enable=True, lora_r=256))
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        check_supported_recipe(_args(lora_enable=True, lora_dropout=0.05))
    with pytest.raises(NotImplementedError, match="lora_bias"):
        check_supported_recipe(_args(lora_enable=True, lora_bias="all"))
    for r in (4, 12, 264, 0):
        with pytest.raises(NotImplementedError, match="lora_r"):
            check_supported_recipe(_args(lora_enable=True, lora_r=r))
    assert lora_config_of(_args()) is None
    assert lora_config_of(_args(lora_enable=True, lora_r=8)) == LoraConfig(r=8, alpha=16.0)
    with pytest.raises(ValueError):
        LoraConfig(r=12)
    with pytest.raises(NotImplementedError):
        LoraConfig(r=8, dropout=0.05)
    with pytest.raises(NotImplementedError):
        LoraConfig(r=8, bias="lora_only")
    with pytest.raises(ValueError):
        LoraConfig(r=8, target_modules=("lm_head",))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _small_table(rank):
    """The gradient-exchange half of a frozen-base HipLlamaTrainer over a LoRA-sized table on the CPU: allreduce_grads touches no
    kernel, so the object is built without an engine and given only the table."""
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    tr = HipLlamaTrainer.__new__(HipLlamaTrainer)
    names = [f"layers.{i}.{m}.lora_{ab}" for i in range(2) for m in ("q_proj", "v_proj") for ab in ("At", "B")] + ["embed", "proj_w", "proj_b"]
    sizes = [64 * 64] * 8 + [128 * 32, 32 * 24, 32]
    tr.frozen = True
    tr.grad_comm = torch.float32
    tr.flat_grad = torch.arange(sum(sizes), dtype=torch.float32) * (rank + 1)
    tr.params, tr.grads, tr._slices, off = [], {}, {}, 0
    for n, sz in zip(names, sizes):
        tr.params.append((n, torch.zeros(sz)))
        tr.grads[n] = tr.flat_grad[off: off + sz]
        tr._slices[n] = (off, sz)
        off += sz
    tr._fresh = set()
    tr._norm_spans = [(0, 5)]
    return tr


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from llark_amd import dist as D

    D.init(backend="gloo")
    tr = _small_table(rank)
    span = tr._layer_span(1)
    tr._start_layer_allreduce(1)                       # layer 1's adapters leave early, as during the backward
    tr.allreduce_grads(world, bucket_elems=5000)       # the rest in small buckets
    q.put((rank, span, tr.flat_grad.tolist(), list(tr._norm_spans)))   # (plain lists: the worker exits right after)
    D.shutdown(world)


def test_two_rank_allreduce_over_the_small_gradient_table():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n = 8 * 64 * 64 + 128 * 32 + 32 * 24 + 32
    want = torch.arange(n, dtype=torch.float32) * 3.0                       # rank 0's + rank 1's, every element exactly once
    for rank, span, flat, spans in res:
        assert span == (4 * 64 * 64, 8 * 64 * 64)                           # layer 1's four adapter tensors, contiguous
        assert torch.equal(torch.tensor(flat), want)
        assert spans == []                                                   # sums of squares taken before the exchange are dropped


def test_load_lora_adapter_from_a_checkpoint_folder_with_a_resized_embedding(tmp_path):
    """A run's checkpoint folder as it is written: adapter files + non_lora_trainables.bin whose embed_tokens has the rows of the added
    audio tokens and whose projector the base model does not have yet.  load_lora_adapter brings the model to those shapes, merges
    W + (alpha / r) B A and takes the trained tensors; a checkpoint with FEWER embedding rows is refused by name."""
    from llark_amd.m2t import lora as LO
    from llark_amd.m2t.llamav2 import WrappedLlamav2Config, WrappedLlamav2ForCausalLM
    H, I, V, MM = 64, 128, 40, 24
    cfg = WrappedLlamav2Config(hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                               vocab_size=V, max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    model = WrappedLlamav2ForCausalLM(cfg)
    base = {k: v.clone() for k, v in model.state_dict().items()}
    lc = LO.LoraConfig(r=8, alpha=16)
    g = torch.Generator().manual_seed(1)
    ad = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in LO.init_adapters(lc, H, I, 1, seed=0).items()}
    folder = tmp_path / "checkpoint-1"
    LO.save_adapter(str(folder), ad, lc)
    extra = {"model.embed_tokens.weight": torch.randn(V + 3, H, generator=g), "model.mm_projector.weight": torch.randn(H, MM, generator=g),
             "model.mm_projector.bias": torch.randn(H, generator=g)}
    torch.save(extra, str(folder / LO.NON_LORA_TRAINABLES))
    model.load_lora_adapter(str(folder))
    now = model.state_dict()
    for k, v in extra.items():
        assert torch.equal(now[k], v), k
    assert now["lm_head.weight"].shape[0] == V + 3 and torch.equal(now["lm_head.weight"][:V], base["lm_head.weight"])
    wk = LO.hf_weight_key(0, "up_proj")
    want = base[wk].double() + lc.scale * (ad[LO.peft_key(0, "up_proj", "B")].double() @ ad[LO.peft_key(0, "up_proj", "A")].double())
    assert torch.allclose(now[wk].double(), want, rtol=0, atol=1e-6)
    assert torch.equal(now["model.norm.weight"], base["model.norm.weight"])
    torch.save({"model.embed_tokens.weight": torch.zeros(V - 1, H)}, str(folder / LO.NON_LORA_TRAINABLES))
    with pytest.raises(ValueError, match="fewer than the base model"):
        WrappedLlamav2ForCausalLM(cfg).load_lora_adapter(str(folder))
