"""MPT backbone on the HIP kernels vs the oracle (itself pinned against the real reference MPTBlock / ALiBi bias):
SURVEY section 8(f) row 2."""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import report_close

pytestmark = pytest.mark.gpu

BASE = dict(d_model=256, n_heads=2, n_layers=2, expansion_ratio=4, vocab_size=96, max_seq_len=128, mm_hidden_size=64)


def _engine(spec, w, precision, max_batch=2, max_seq=64):
    from llark_amd.m2t.mpt_engine import HipMptEngine, MptDims
    dims = MptDims(d_model=spec.d_model, n_heads=spec.n_heads, n_layers=spec.n_layers, expansion_ratio=spec.expansion_ratio,
                   vocab_size=spec.vocab_size, max_seq_len=spec.max_seq_len, alibi_bias_max=spec.alibi_bias_max, qk_ln=spec.qk_ln,
                   clip_qkv=spec.clip_qkv, logit_scale=spec.logit_scale, ln_eps=spec.ln_eps, mm_hidden_size=spec.mm_hidden_size)
    eng = HipMptEngine(dims, "cuda", max_batch, max_seq, precision=precision)
    eng.load_state_dict(w)
    return eng


@pytest.mark.parametrize("case", ["alibi", "alibi+qk_ln+clip+bias+logit_scale"])
def test_mpt_engine_split_matches_oracle(case):
    """fp32-class mode: logits, hidden state and cached decode steps vs the fp32 oracle (tolerance 1e-4 of max|ref|;
    measured ~2e-5), with the audio splice through mm_projector."""
    from oracle import mpt_ref as MR
    extra = {} if case == "alibi" else dict(qk_ln=True, clip_qkv=0.75, no_bias=False, alibi_bias_max=4, logit_scale=0.5)
    spec = MR.MptSpec(**BASE, audio_start_token=93, audio_end_token=94, audio_patch_token=95, **extra)
    w = MR.make_weights(spec, seed=7)
    g = torch.Generator().manual_seed(2)
    B, S = 2, 29
    ids = torch.randint(0, 90, (B, S), generator=g)
    ids[:, 2], ids[:, 3:8], ids[:, 8] = 93, 95, 94
    aud = torch.randn(B, 5, 64, generator=g)
    ref = MR.forward(w, spec, ids, aud, return_hidden=True)
    eng = _engine(spec, w, "split")
    segs = [(b, 2, aud[b].cuda()) for b in range(B)]
    logits = eng.forward_tokens(ids.cuda(), segs)
    report_close("mpt logits (split) vs oracle", logits.cpu(), ref["logits"], 1e-4 * ref["logits"].abs().max().item())
    # cached decode: 4 steps, each compared with the oracle run on the growing cache
    past = ref["past_key_values"]
    for step in range(4):
        tok = torch.randint(0, 90, (B, 1), generator=g)
        r = MR.forward(w, spec, tok, None, past_key_values=past)
        past = r["past_key_values"]
        lg = eng.forward_tokens(tok.cuda(), (), pos0=eng.cur_len)
        report_close(f"mpt decode step {step}", lg.cpu(), r["logits"], 1e-4 * r["logits"].abs().max().item())
    assert eng.cur_len == S + 4
    # last_only prefill == last row of the full prefill
    lo = eng.forward_tokens(ids.cuda(), segs, last_only=True)
    report_close("last_only", lo[:, 0].cpu(), ref["logits"][:, -1], 1e-4 * ref["logits"].abs().max().item())


def test_mpt_engine_bf16_flow_and_errors():
    """Single-pass mode stays within bf16-flow distance of the fp32 oracle; sequence longer than the cache raises."""
    from oracle import mpt_ref as MR
    spec = MR.MptSpec(**BASE)
    w = MR.make_weights(spec, seed=9)
    ids = torch.randint(0, 96, (2, 40), generator=torch.Generator().manual_seed(4))
    ref = MR.forward(w, spec, ids)["logits"]
    eng = _engine(spec, w, "bf16")
    lg = eng.forward_tokens(ids.cuda())
    rel = (lg.cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert rel < 3e-2, rel
    assert (lg.cpu().argmax(-1) == ref.argmax(-1)).float().mean().item() > 0.9
    with pytest.raises(ValueError, match="Cannot forward input"):
        eng.forward_tokens(torch.zeros((2, 65), dtype=torch.int64, device="cuda"))
    with pytest.raises(NotImplementedError):
        from llark_amd.m2t.mpt_engine import HipMptEngine, MptDims
        HipMptEngine(MptDims(d_model=256, n_heads=4), "cuda")               # head_dim 64


def test_mpt_1b_width_two_blocks():
    """MPT-1B widths (d_model 2048, 16 heads, expansion 4, ALiBi), 2 blocks, S = 371-like prompt, small vocab."""
    from oracle import mpt_ref as MR
    spec = MR.MptSpec(d_model=2048, n_heads=16, n_layers=2, expansion_ratio=4, vocab_size=512, max_seq_len=2048, mm_hidden_size=512,
                      audio_start_token=509, audio_end_token=510, audio_patch_token=511)
    w = MR.make_weights(spec, seed=1, std=0.02)
    g = torch.Generator().manual_seed(0)
    B, S = 2, 131
    ids = torch.randint(0, 500, (B, S), generator=g)
    ids[:, 1], ids[:, 2], ids[:, 3] = 509, 511, 510                         # CLAP-style: ONE 512-d frame per clip (F = 1)
    aud = torch.randn(B, 1, 512, generator=g)
    ref = MR.forward(w, spec, ids, aud)["logits"]
    eng = _engine(spec, w, "split", max_batch=B, max_seq=192)
    lg = eng.forward_tokens(ids.cuda(), [(b, 1, aud[b].cuda()) for b in range(B)])
    report_close("mpt-1b width logits vs oracle", lg.cpu(), ref, 1e-4 * ref.abs().max().item())


def test_wrapped_mpt_surface_forward_generate_errors():
    """The reference surface (m2t/models/mpt.py): state-dict names, forward with audio splice (start/end AND the
    patch-token branch :190-232), loss, greedy generate through prepare_inputs_for_generation, tokenizer set-up, errors."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from toy_tokenizer import ToyTokenizer
    from llark_amd.m2t.mpt import WrappedMPTConfig, WrappedMPTForCausalLM
    from oracle import mpt_ref as MR
    spec = MR.MptSpec(**BASE, audio_start_token=93, audio_end_token=94, audio_patch_token=95)
    w = MR.make_weights(spec, seed=21)
    cfg = WrappedMPTConfig(d_model=256, n_heads=2, n_layers=2, expansion_ratio=4, max_seq_len=128, vocab_size=96, mm_hidden_size=64)
    m = WrappedMPTForCausalLM(cfg)
    missing = m.load_state_dict(w, strict=True)                               # the reference's names, nothing missing / unexpected
    ac = m.get_model().audio_encoder_config
    ac.use_audio_start_end, ac.audio_start_token, ac.audio_end_token, ac.audio_patch_token = True, 93, 94, 95
    with pytest.raises(Exception, match="GPU"):
        m(input_ids=torch.zeros((1, 4), dtype=torch.long))                     # CPU model: loud, no fallback
    m.cuda().eval()
    m.configure_engine(max_batch=2, max_seq=96)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 90, (2, 23), generator=g)
    ids[:, 1], ids[:, 2:6], ids[:, 6] = 93, 95, 94
    aud = torch.randn(2, 4, 64, generator=g)
    lab = ids.clone()
    lab[:, :8] = -100
    ref = MR.forward(w, spec, ids, aud, labels=lab)
    with torch.no_grad():
        out = m(input_ids=ids.cuda(), audio_encodings=aud.cuda(), labels=lab.cuda())
    report_close("wrapped mpt logits", out.logits.cpu(), ref["logits"], 1e-4 * ref["logits"].abs().max().item())
    assert abs(out.loss.item() - ref["loss"].item()) < 1e-4 * max(1.0, ref["loss"].item())
    # list-of-tensors encodings take the same path
    with torch.no_grad():
        out_l = m(input_ids=ids.cuda(), audio_encodings=[aud[0].cuda(), aud[1].cuda()])
    assert torch.equal(out_l.logits, out.logits)
    # patch-token branch (use_audio_start_end = False): the frames replace exactly the <audio_patch> run
    ac.use_audio_start_end = False
    ids_p = ids.clone()
    ids_p[:, 1], ids_p[:, 6] = 5, 6                                            # no start / end tokens any more
    x = torch.nn.functional.embedding(ids_p, w["transformer.wte.weight"])
    x[:, 2:6] = torch.nn.functional.linear(aud, w["transformer.mm_projector.weight"], w["transformer.mm_projector.bias"])
    h = x
    for i in range(spec.n_layers):
        h, _ = MR.block(w, spec, i, h, None)
    ref_p = torch.nn.functional.linear(torch.nn.functional.layer_norm(h, (256,), w["transformer.norm_f.weight"], None, 1e-5), w["transformer.wte.weight"])
    with torch.no_grad():
        out_p = m(input_ids=ids_p.cuda(), audio_encodings=aud.cuda())
    report_close("patch-branch logits", out_p.logits.cpu(), ref_p, 1e-4 * ref_p.abs().max().item())
    bad = ids_p.clone()
    bad[0, 4] = 7                                                              # only 3 patch tokens for 4 frames
    with pytest.raises(ValueError, match="number of audio patch tokens"):
        m(input_ids=bad.cuda(), audio_encodings=aud.cuda())
    gap = ids_p.clone()
    gap[0, 5], gap[0, 9] = 7, 95                                               # 4 patch tokens, not consecutive
    with pytest.raises(ValueError, match="consecutive"):
        m(input_ids=gap.cuda(), audio_encodings=aud.cuda())
    ac.use_audio_start_end = True
    # greedy generate == oracle greedy (prompt with audio once, then cached single-token steps)
    gen = m.generate(input_ids=ids.cuda(), audio_encodings=aud.cuda(), max_new_tokens=6).cpu()
    ref_gen = MR.greedy_generate(w, spec, ids, aud, 6)
    assert torch.equal(gen, ref_gen), (gen[:, -6:].tolist(), ref_gen[:, -6:].tolist())
    with pytest.raises(NotImplementedError, match="right padding"):
        m.prepare_inputs_for_generation(ids, attention_mask=torch.tensor([[1] * 22 + [0]] * 2))
    # tokenizer set-up: 3 new rows, start/end rows = mean of the earlier rows (tied table)
    tok = ToyTokenizer()
    for t in ("a b c d e f g",):
        tok.encode(t)
    m2 = WrappedMPTForCausalLM(WrappedMPTConfig(d_model=256, n_heads=2, n_layers=1, expansion_ratio=4, max_seq_len=64, vocab_size=len(tok), mm_hidden_size=64))
    base = len(tok)
    m2.initialize_audio_tokenizer(True, tok, "cpu")
    emb = m2.get_input_embeddings().weight.data
    assert emb.shape[0] == base + 3 and torch.allclose(emb[-2:], emb[:-2].mean(0, keepdim=True).expand(2, -1), atol=1e-6)
    a2 = m2.get_model().audio_encoder_config
    assert (a2.audio_patch_token, a2.audio_start_token, a2.audio_end_token) == tuple(tok.convert_tokens_to_ids(["<audio_patch>", "<audio_start>", "<audio_end>"]))


@pytest.mark.parametrize("case", ["alibi", "alibi+qk_ln+bias", "alibi+qk_ln+clip+bias+logit_scale", "alibi+clip"])
def test_mpt_training_step_gradients_match_autograd(case):
    """HipMptTrainer (forward with saved activations, full backward, AdamW) vs torch autograd of the fp32 oracle on bf16-valued
    weights: per-tensor relative Frobenius error <= 5e-2 and cosine >= 0.995 (bf16 operands in both passes), loss within 1 %;
    then a few optimizer steps reduce the loss."""
    from llark_amd.m2t.mpt_train_engine import HipMptTrainer
    from oracle import mpt_ref as MR
    extra = {"alibi": {}, "alibi+qk_ln+bias": dict(qk_ln=True, no_bias=False, alibi_bias_max=4),
             "alibi+qk_ln+clip+bias+logit_scale": dict(qk_ln=True, clip_qkv=3.0, no_bias=False, alibi_bias_max=4, logit_scale=0.5),
             "alibi+clip": dict(clip_qkv=3.2)}[case]
    # clip at ~2.5 sigma of these weights' qkv (sigma ~ 0.08 sqrt(256) = 1.28): about 1 % of the entries are cut -- a missing mask
    # would be a ~10 % gradient error, an inverted one ~100 % -- while few entries sit within the bf16 rounding of the threshold
    # (the GPU's qkv comes from bf16 activations, the oracle's from fp32: at a clip of 0.4 sigma the entries that land on different
    # sides of it are a 5.5 % gradient difference by themselves, measured)
    spec = MR.MptSpec(**BASE, audio_start_token=93, audio_end_token=94, audio_patch_token=95, **extra)
    w = MR.make_weights(spec, seed=31, std=0.08)
    g = torch.Generator().manual_seed(8)
    B, S = 2, 24
    ids = torch.randint(0, 90, (B, S), generator=g)
    ids[:, 2], ids[:, 3:7], ids[:, 7] = 93, 95, 94
    aud = torch.randn(B, 4, 64, generator=g)
    labels = ids.clone()
    labels[:, :9] = -100
    wp = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    ref = MR.forward(wp, spec, ids, aud, labels=labels)
    ref["loss"].backward()
    eng = _engine(spec, w, "bf16", max_batch=B, max_seq=64)
    tr = HipMptTrainer(eng, lr=2e-3, train_wte=True)
    segs = [(b, 2, aud[b].cuda()) for b in range(B)]
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda())
    assert abs(loss.item() - ref["loss"].item()) <= 1e-2 * max(1.0, ref["loss"].item())
    got = tr.export_grads_ref()
    worst = {}
    biggest = max(p_.grad.norm().item() for p_ in wp.values() if p_.grad is not None)
    for name, gg in got.items():
        r = wp[name].grad
        a, b_ = gg.float().cpu().reshape(-1), r.reshape(-1)
        if b_.norm().item() < 1e-4 * biggest:        # e.g. k_ln.bias: a constant added to every key cancels in the softmax -> exact 0
            assert a.norm().item() < 1e-2 * biggest, f"{name}: reference gradient ~0 but got norm {a.norm().item():.3e}"
            continue
        rel = ((a - b_).norm() / (b_.norm() + 1e-12)).item()
        cos = (torch.dot(a, b_) / (a.norm() * b_.norm() + 1e-20)).item()
        worst[name] = (rel, cos)
        assert rel <= 5e-2 and cos >= 0.995, f"{name}: rel {rel:.3e} cos {cos:.5f}"
    print("worst mpt grad rel errs:", sorted(((v[0], k) for k, v in worst.items()), reverse=True)[:3])
    assert set(got) == {k for k in w}                                        # every reference parameter has a gradient
    l0 = loss.item()
    tr.step()
    for _ in range(5):
        l1 = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
        tr.step()
    assert l1 < 0.8 * l0, (l0, l1)
    # the frozen-wte recipe (reference default) has no wte gradient slot
    tr2 = HipMptTrainer(_engine(spec, w, "bf16", max_batch=B, max_seq=64))
    assert "transformer.wte.weight" not in tr2.export_grads_ref()


def _compare_grads_with_autograd(got, wp):
    """the whole-model bound of test_mpt_training_step_gradients_match_autograd: per-tensor relative Frobenius error <= 5e-2 and
    cosine >= 0.995; tensors whose reference gradient is < 1e-4 of the largest must be small on the GPU too"""
    worst = {}
    biggest = max(p_.grad.norm().item() for p_ in wp.values() if p_.grad is not None)
    for name, gg in got.items():
        a, b_ = gg.float().cpu().reshape(-1), wp[name].grad.reshape(-1)
        if b_.norm().item() < 1e-4 * biggest:
            assert a.norm().item() < 1e-2 * biggest, f"{name}: reference gradient ~0 but got norm {a.norm().item():.3e}"
            continue
        rel = ((a - b_).norm() / (b_.norm() + 1e-12)).item()
        cos = (torch.dot(a, b_) / (a.norm() * b_.norm() + 1e-20)).item()
        worst[name] = (rel, cos)
        assert rel <= 5e-2 and cos >= 0.995, f"{name}: rel {rel:.3e} cos {cos:.5f}"
    print("worst mpt grad rel errs:", sorted(((v[0], k) for k, v in worst.items()), reverse=True)[:3])
    assert set(got) == set(wp)


@pytest.mark.parametrize("V,S,bias", [(50371, 96, True), (50432, 93, False), (4099, 93, True), (4160, 96, False)],
                         ids=["V50371-S96-bias", "V50432-S93", "V4099-S93-bias", "V4160-S96"])
def test_mpt_training_step_at_1b_width_takes_the_recipe_branches(monkeypatch, V, S, bias):
    """The gradient test at MPT-1B width (d_model 2048, 16 heads, expansion 4, qk_ln: layernorm_bwd NV = 8 on full rows and on
    column slices, colsum / gelu_bwd at 8192 columns), 2 blocks.  B S = 192 rows (a multiple of 64: every dW goes through
    gemm16_t on the operands as stored) and 186 rows (the transposed16 fallback); a vocabulary that is a multiple of 64 (dX of the
    tied wte through gemm16_t) and one that is not (the padded fallback).  Which branch ran is asserted, not assumed."""
    from llark_amd import ops
    from llark_amd.m2t.mpt_train_engine import HipMptTrainer
    from oracle import mpt_ref as MR
    a0 = 50368 if V > 50000 else 4096                                       # the three audio tokens follow the text vocabulary
    spec = MR.MptSpec(d_model=2048, n_heads=16, n_layers=2, expansion_ratio=4, vocab_size=V, max_seq_len=128, mm_hidden_size=64,
                      qk_ln=True, no_bias=not bias, audio_start_token=a0, audio_end_token=a0 + 1, audio_patch_token=a0 + 2)
    w = MR.make_weights(spec, seed=5, std=0.02)
    g = torch.Generator().manual_seed(9)
    B = 2
    ids = torch.randint(0, a0, (B, S), generator=g)
    ids[:, 2], ids[:, 3:7], ids[:, 7] = a0, a0 + 2, a0 + 1
    aud = torch.randn(B, 4, 64, generator=g)
    labels = ids.clone()
    labels[:, :9] = -100
    wp = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    ref = MR.forward(wp, spec, ids, aud, labels=labels)
    ref["loss"].backward()
    eng = _engine(spec, w, "bf16", max_batch=B, max_seq=128)
    tr = HipMptTrainer(eng, train_wte=True)
    calls = {"dw_t": 0, "dx_wte_t": 0, "transposed16": 0}
    rows = B * S
    real_t, real_tr = ops.gemm16_t, ops.transposed16

    def counting_gemm16_t(a, wt, m, n, kp, trans_a, trans_b, c, **kw):
        if trans_a and kp == rows:
            calls["dw_t"] += 1
        if not trans_a and kp == V:
            calls["dx_wte_t"] += 1
        return real_t(a, wt, m, n, kp, trans_a, trans_b, c, **kw)

    def counting_transposed16(x, *a, **kw):
        calls["transposed16"] += 1
        return real_tr(x, *a, **kw)

    monkeypatch.setattr(ops, "gemm16_t", counting_gemm16_t)
    monkeypatch.setattr(ops, "transposed16", counting_transposed16)
    loss = tr.forward_backward(ids.cuda(), [(b, 2, aud[b].cuda()) for b in range(B)], labels.cuda())
    n_dw = 4 * spec.n_layers + 1                                            # Wqkv, out_proj, up, down per block + the tied wte
    if rows % 64 == 0:
        # wte's dW operand has V columns: gemm16_t needs V % 8 == 0, else that one product transposes
        assert calls["dw_t"] == n_dw - (1 if V % 8 else 0), calls
    else:
        assert calls["dw_t"] == 0 and calls["transposed16"] >= 2 * n_dw, calls
    assert calls["dx_wte_t"] == (1 if V % 64 == 0 else 0), calls
    assert abs(loss.item() - ref["loss"].item()) <= 1e-2 * max(1.0, ref["loss"].item())
    _compare_grads_with_autograd(tr.export_grads_ref(), wp)


def test_mpt_trainer_accumulates_gradients_over_micro_batches():
    """Two forward_backward calls without zero_grad leave the SUM of the two gradients in every slot (weights, biases, LayerNorm
    gains and shifts, q/k LayerNorm, projector, tied wte): every dgamma / dbeta / bias kernel adds into its slot.  The two passes
    are the same launches as the separate ones, so only the fp32 summation order of the atomically accumulated slots can differ:
    <= 256 * 2**-24 of the larger addend per tensor (sums of <= 96 terms), while an overwritten slot would be off by a whole addend."""
    from llark_amd.m2t.mpt_train_engine import HipMptTrainer
    from oracle import mpt_ref as MR
    spec = MR.MptSpec(**BASE, audio_start_token=93, audio_end_token=94, audio_patch_token=95, qk_ln=True, clip_qkv=3.0, no_bias=False,
                      alibi_bias_max=4, logit_scale=0.5)
    w = MR.make_weights(spec, seed=31, std=0.08)
    g = torch.Generator().manual_seed(10)
    B, S = 2, 24
    batches = []
    for _ in range(2):
        ids = torch.randint(0, 90, (B, S), generator=g)
        ids[:, 2], ids[:, 3:7], ids[:, 7] = 93, 95, 94
        aud = torch.randn(B, 4, 64, generator=g)
        labels = ids.clone()
        labels[:, :9] = -100
        batches.append((ids.cuda(), [(b, 2, aud[b].cuda()) for b in range(B)], labels.cuda()))
    tr = HipMptTrainer(_engine(spec, w, "bf16", max_batch=B, max_seq=64), train_wte=True)
    single = []
    for bt in batches:
        tr.zero_grad()
        tr.forward_backward(*bt)
        single.append({k: v.clone() for k, v in tr.grads.items()})
    tr.zero_grad()
    for bt in batches:
        tr.forward_backward(*bt)
    for name, got in tr.grads.items():
        g1, g2 = single[0][name].double().cpu(), single[1][name].double().cpu()
        assert g1.abs().max().item() > 0 or name.endswith("klb"), f"{name}: no gradient reached this slot"
        report_close(f"accumulated {name}", got.double().cpu(), g1 + g2, 256 * 2.0 ** -24 * max(g1.abs().max().item(), g2.abs().max().item()))
