"""GPU parity of the packed ragged training step (``HipLlamaTrainer.forward_backward_packed``): a whole optimizer step of sequences of
different lengths as ONE row stream, on the variable-length attention kernels, against torch autograd over the oracle.

The oracle is called once per micro-batch on that micro-batch's sequences right-padded with label -100 (which it handles as it
stands); the loss is the mean of the micro-batch means.  Bars are the project's own (tests/test_train_gpu.py): loss within
5e-3 max(1, |ref|); every trainable tensor within relative Frobenius error 3e-2 and cosine 0.999.  Dimensions and helpers follow
tests/test_lora_train_gpu.py.  Two setups: lengths (72, 40, 23, 56) in micro-batches (2, 2) -- 192 packed rows, the fragment-major twin
path with every fused epilogue -- and lengths (20, 13) in (1, 1) -- 40 packed rows, below FRAG_MIN_ROWS: the unfused path with
rope_split_heads on the gathered RoPE table.  The shipped loop (one right-padded ``forward_backward`` per micro-batch) runs on the
same examples and is held to the same oracle under the same bars; the difference between the two HIP gradients is printed."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, H, I, NH, LAYERS, MM = 128, 256, 512, 2, 2, 96
F = 5                         # audio frames per example
PAD_ID = 0
TOKS = (V - 2, V - 1)
CASES = {"twins": ((72, 40, 23, 56), (2, 2)), "small": ((20, 13), (1, 1))}


def _bf(x):
    return x.bfloat16().float()


@functools.lru_cache(maxsize=None)
def _data(case):
    """weights + the examples of one optimizer step: 1-D ids / labels per example, one audio clip each"""
    from oracle import llama_ref as LR
    lengths, groups = CASES[case]
    spec = LR.LlamaSpec(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH, vocab_size=V,
                        mm_hidden_size=MM, audio_start_token=V - 2, audio_end_token=V - 1, audio_patch_token=V - 3)
    w = {k: _bf(v) for k, v in LR.make_weights(spec, seed=0, std=0.08).items()}
    g = torch.Generator().manual_seed(6)
    ids, labels = [], []
    for b, n in enumerate(lengths):
        head = 1 + b % 2
        t = torch.tensor([1] + torch.randint(3, V - 3, (head,), generator=g).tolist() + [V - 2] + [V - 3] * F + [V - 1]
                         + torch.randint(3, V - 3, (n - F - 3 - head,), generator=g).tolist())
        assert t.shape == (n,)
        lab = t.clone()
        lab[:9] = -100
        ids.append(t)
        labels.append(lab)
    aud = torch.randn(len(lengths), F, MM, generator=g)
    return spec, w, ids, labels, aud, groups


def _micro_batches(case):
    """the step as the shipped loop sees it: per micro-batch (ids [B][S], labels, audio [B][F][MM]) right-padded to its longest example"""
    spec, w, ids, labels, aud, groups = _data(case)
    out, b0 = [], 0
    for gsize in groups:
        S = max(int(t.numel()) for t in ids[b0:b0 + gsize])
        mi = torch.full((gsize, S), PAD_ID, dtype=torch.long)
        ml = torch.full((gsize, S), -100, dtype=torch.long)
        for j in range(gsize):
            n = int(ids[b0 + j].numel())
            mi[j, :n], ml[j, :n] = ids[b0 + j], labels[b0 + j]
        out.append((mi, ml, aud[b0:b0 + gsize]))
        b0 += gsize
    return out


def _start(t):
    return int((t == V - 2).nonzero()[0, 0])


def _trainer(case, r=None, **kw):
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    spec, w, ids, labels, aud, groups = _data(case)
    dims = LlamaDims(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH, vocab_size=V, mm_hidden_size=MM)
    eng = HipLlamaEngine(dims, "cuda", 2, 128, precision="bf16")
    eng.load_state_dict(w)
    if r is not None:
        cfg, ad = _adapters(r)
        tr = HipLlamaTrainer(eng, embed_grad_tokens=TOKS, lora=cfg, **kw)
        tr.set_adapters(ad)
        return tr
    return HipLlamaTrainer(eng, embed_grad_tokens=TOKS, **kw)


def _run_packed(tr, case):
    spec, w, ids, labels, aud, groups = _data(case)
    segs = [(b, _start(t), aud[b].cuda()) for b, t in enumerate(ids)]
    return tr.forward_backward_packed(ids, segs, labels, groups, pad_id=PAD_ID).item()


def _run_loop(tr, case):
    """the shipped loop: one right-padded forward_backward per micro-batch, gradients accumulated"""
    mbs = _micro_batches(case)
    loss = 0.0
    for mi, ml, ma in mbs:
        segs = [(b, _start(mi[b]), ma[b].cuda()) for b in range(mi.shape[0])]
        loss += tr.forward_backward(mi.cuda(), segs, ml.cuda(), 1.0 / len(mbs)).item() / len(mbs)
    return loss


@functools.lru_cache(maxsize=None)
def _adapters(r, b_std=0.02):
    from llark_amd.m2t import lora as LO
    cfg = LO.LoraConfig(r=r, alpha=16)
    ad = LO.init_adapters(cfg, H, I, LAYERS, seed=3)
    g = torch.Generator().manual_seed(11)
    for k in ad:
        ad[k] = _bf(torch.randn(ad[k].shape, generator=g) * b_std) if ".lora_B." in k else _bf(ad[k])
    return cfg, ad


@functools.lru_cache(maxsize=None)
def _oracle(case, r=None):
    """(loss, gradients): autograd over the oracle, once per micro-batch on its right-padded sequences; the mean of the micro-batch means.
    r: LoRA rank (W_eff = W + s B A, the adapter factors are the leaves); None: every weight is a leaf."""
    from llark_amd.m2t import lora as LO
    from oracle import llama_ref as LR
    spec, w = _data(case)[:2]
    wp = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    leaves = dict(wp)
    if r is not None:
        cfg, ad = _adapters(r)
        leaves = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
        for k in ("model.embed_tokens.weight", "model.mm_projector.weight", "model.mm_projector.bias"):
            leaves[k] = wp[k]
        for i in range(LAYERS):
            for mod in LO.TARGET_MODULES:
                wk = LO.hf_weight_key(i, mod)
                wp[wk] = w[wk] + cfg.scale * (leaves[LO.peft_key(i, mod, "B")] @ leaves[LO.peft_key(i, mod, "A")])
    mbs = _micro_batches(case)
    loss = sum(LR.forward(wp, spec, mi, ma, labels=ml, act_dtype=torch.bfloat16, round_probs=True)["loss"] for mi, ml, ma in mbs) / len(mbs)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in leaves.items()}


def _check(tag, loss, got, ref_loss, ref):
    print(f"{tag}: loss {loss:.6f} ref {ref_loss:.6f}")
    assert abs(loss - ref_loss) <= 5e-3 * max(1.0, abs(ref_loss)), (tag, loss, ref_loss)
    worst = {}
    for name, gh in got.items():
        r = ref[name]
        gh = gh.float().cpu()
        if name == "model.embed_tokens.weight":
            others = [i for i in range(V) if i not in TOKS]                   # the pad id's row among them
            assert gh[others].abs().max().item() == 0.0, f"{tag}: an embedding row other than the audio tokens' got a gradient"
            gh, r = gh[list(TOKS)], r[list(TOKS)]
        rel = ((gh - r).norm() / (r.norm() + 1e-30)).item()
        cos = torch.nn.functional.cosine_similarity(gh.flatten(), r.flatten(), dim=0).item()
        worst[name] = (rel, cos)
    top = sorted(worst.items(), key=lambda kv: -kv[1][0])[:4]
    print(f"{tag}: worst grad rel errs:", [(k, f"{v[0]:.2e}", f"{v[1]:.5f}") for k, v in top])
    for name, (rel, cos) in worst.items():
        assert np.isfinite(rel) and rel <= 3e-2 and cos >= 0.999, f"{tag}: {name}: rel {rel:.3e} cos {cos:.5f}"


def _count_launches(monkeypatch):
    from llark_amd import ops
    launches = {nm: 0 for nm in ("gemm16_fragw_rope_qkv_train", "gemm16_fragw_swiglu_train", "rope_split_heads", "swiglu_fwd",
                                 "attn_prefill_lse_varlen", "attn_backward_fused_varlen", "attn_backward_varlen",
                                 "attn_prefill_lse", "attn_prefill", "attn_backward_fused", "attn_backward")}
    for nm in launches:
        def counted(*a, _nm=nm, _fn=getattr(ops, nm), **kw):
            launches[_nm] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, nm, counted)
    return launches


@pytest.mark.parametrize("case", list(CASES))
def test_packed_step_matches_autograd_and_the_shipped_loop(case, monkeypatch):
    launches = _count_launches(monkeypatch)
    tr = _trainer(case)
    loss = _run_packed(tr, case)
    uniform = dict(attn_prefill_lse=0, attn_prefill=0, attn_backward_fused=0, attn_backward=0)      # no uniform attention entry point ran
    if case == "twins":       # 192 rows: fused RoPE q|k|v epilogue, fused SwiGLU products, the fused variable-length backward
        assert launches == dict(gemm16_fragw_rope_qkv_train=LAYERS, gemm16_fragw_swiglu_train=2 * LAYERS, rope_split_heads=0, swiglu_fwd=0,
                                attn_prefill_lse_varlen=LAYERS, attn_backward_fused_varlen=LAYERS, attn_backward_varlen=0, **uniform), launches
    else:                     # 40 rows, below FRAG_MIN_ROWS: rope_split_heads on the gathered table, the unfused variable-length backward
        assert launches == dict(gemm16_fragw_rope_qkv_train=0, gemm16_fragw_swiglu_train=0, rope_split_heads=LAYERS, swiglu_fwd=LAYERS,
                                attn_prefill_lse_varlen=LAYERS, attn_backward_fused_varlen=0, attn_backward_varlen=LAYERS, **uniform), launches
    ref_loss, ref = _oracle(case)
    got = {k: v.float().cpu().clone() for k, v in tr.export_grads_hf().items()}
    assert set(got) == set(ref) - {"lm_head.weight"}                           # lm_head is frozen like the reference's
    _check(f"packed {case}", loss, got, ref_loss, ref)
    # the shipped loop on the same examples: the same oracle, the same bars
    tr2 = _trainer(case)
    loss2 = _run_loop(tr2, case)
    got2 = {k: v.float().cpu().clone() for k, v in tr2.export_grads_hf().items()}
    _check(f"loop {case}", loss2, got2, ref_loss, ref)
    rel = max(((got[k] - got2[k]).norm() / (got2[k].norm() + 1e-30)).item() for k in got)
    print(f"packed vs shipped loop, {case}: loss {loss:.6f} vs {loss2:.6f}; worst relative difference of a gradient tensor {rel:.3e}")


@pytest.mark.parametrize("mode", ["lora", "freeze_backbone"])
def test_packed_step_frozen_base_recipes(mode):
    from llark_amd.m2t import lora as LO
    r = 8 if mode == "lora" else None
    tr = _trainer("twins", r) if r is not None else _trainer("twins", freeze_backbone=True)
    loss = _run_packed(tr, "twins")
    ref_loss, ref = _oracle("twins", r)
    got = tr.export_grads_hf()
    want = {"model.embed_tokens.weight", "model.mm_projector.weight", "model.mm_projector.bias"}
    if r is not None:
        want |= {LO.peft_key(i, m, ab) for i in range(LAYERS) for m in LO.TARGET_MODULES for ab in "AB"}
    assert set(got) == want                                                   # nothing for a frozen tensor
    _check(f"packed {mode}", loss, got, ref_loss, ref)


def test_packed_step_with_gradient_checkpointing_is_bit_equal():
    """the backward re-runs each layer's forward (variable-length attention, gathered RoPE table, cache views included) with the same
    kernels in the same order: the same loss and, bit for bit, every gradient the step computes reproducibly -- all weight matrices.
    The RMSNorm gains, the projector bias and the embedding rows are fp32 ATOMIC sums in kernels this step shares with the uniform one
    (rmsnorm_bwd, colsum_add, scatter_add_rows: csrc/train.hip): two runs of the SAME configuration differ in their last bits, so
    for those the comparison is the one tests/test_train_gpu.py makes for the uniform step (rtol 1e-5, atol 1e-7)."""
    tr = _trainer("twins")
    loss = _run_packed(tr, "twins")
    trc = _trainer("twins", gradient_checkpointing=True)
    lossc = _run_packed(trc, "twins")
    assert loss == lossc
    tr._finalize_grads(), trc._finalize_grads()
    for name, prm in tr.params:
        a, b = tr.grads[name], trc.grads[name]
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        print(f"checkpointing {name}: {'bit-equal' if same else f'max abs diff {(a - b).abs().max().item():.3e} of max {a.abs().max().item():.3e}'}")
        if prm.dim() == 2 and name != "embed":
            assert same, name
        else:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), name


def test_packed_step_refuses_what_the_caches_cannot_hold():
    tr = _trainer("small")
    spec, w, ids, labels, aud, groups = _data("small")
    long = [torch.randint(3, V - 3, (120,)) for _ in range(3)]                # 360 rows > max_batch * smax = 2 * 128
    with pytest.raises(ValueError, match="s_total = 360.*max_batch \\* smax"):
        tr.forward_backward_packed(long, [], [t.clone() for t in long], (3,))


def test_train_loop_with_pack_sequences_follows_the_shipped_loop():
    """TrainConfig.pack_sequences through ``train()``: the collated ragged micro-batches (attention_mask, right padding) of each step are
    planned into one stream and run as one pass; the logged losses follow the unpacked loop's under the project's loss bar."""
    from llark_amd.m2t import AudioEncoderConfig
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    from llark_amd.m2t.train import TrainConfig, train
    spec, w = _data("twins")[:2]
    ac = AudioEncoderConfig()
    ac.audio_start_token, ac.audio_end_token, ac.audio_patch_token = spec.audio_start_token, spec.audio_end_token, spec.audio_patch_token
    stream = [dict(input_ids=mi, labels=ml, attention_mask=mi.ne(PAD_ID), audio_encodings=ma) for mi, ml, ma in _micro_batches("twins")] * 3
    dims = LlamaDims(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH, vocab_size=V, mm_hidden_size=MM)

    def run(pack):
        e = HipLlamaEngine(dims, "cuda", 4 if pack else 2, 128, precision="bf16")
        e.load_state_dict(w)
        return train(e, stream, ac, TrainConfig(learning_rate=2e-3, max_steps=20, gradient_accumulation_steps=2, pack_sequences=pack), world=1)

    base, packed = run(False), run(True)
    print("train loop losses:", base, "packed:", packed)
    assert len(base) == len(packed) == 3
    assert all(abs(a - b) <= 5e-3 * max(1.0, abs(a)) for a, b in zip(base, packed)), (base, packed)
    assert packed[-1] < packed[0]
