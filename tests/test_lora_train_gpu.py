"""GPU parity of the frozen-base training modes of ``HipLlamaTrainer``: LoRA adapters (``lora=LoraConfig(...)``, m2t/train.py:82-99) and
``freeze_backbone=True`` (m2t/train.py:79,146-148), against torch autograd over the oracle.

The oracle is not touched: it is given ``W_eff = W + (alpha / r) B A`` for the seven matrices per layer, with A, B, the projector and
the embedding as autograd leaves.  Bars are the project's own (tests/test_train_gpu.py): loss within 5e-3 max(1, |ref|); every
trainable tensor within relative Frobenius error 3e-2 and cosine 0.999.  The two setups are those of tests/test_train_gpu.py: 40 rows
(below FRAG_MIN_ROWS: the products run on W as stored, the adapters as separate low-rank products) and 144 rows (the fragment-major
twins with the adapters in extra K columns: fused RoPE / SwiGLU epilogues kept)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, H, I, NH, LAYERS, MM = 128, 256, 512, 2, 2, 96


def _bf(x):
    return x.bfloat16().float()


@functools.lru_cache(maxsize=None)
def _data(S):
    """Weights + one batch (B = 2): S = 20 is the 40-row shape, S = 72 the 144-row shape."""
    from oracle import llama_ref as LR
    spec = LR.LlamaSpec(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH, vocab_size=V,
                        mm_hidden_size=MM, audio_start_token=V - 2, audio_end_token=V - 1, audio_patch_token=V - 3)
    w = {k: _bf(v) for k, v in LR.make_weights(spec, seed=0, std=0.08).items()}
    g = torch.Generator().manual_seed(6)
    F, B = 5, 2
    ids = torch.stack([torch.tensor([1] + torch.randint(3, V - 3, (2 + b,), generator=g).tolist() + [V - 2] + [V - 3] * F + [V - 1]
                                    + torch.randint(3, V - 3, (S - F - 5 - b,), generator=g).tolist()) for b in range(B)])
    assert ids.shape == (B, S)
    aud = torch.randn(B, F, MM, generator=g)
    labels = ids.clone()
    labels[:, :10] = -100
    return spec, w, ids, aud, labels


def _engine(S, w=None, max_seq=128):
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    spec, w0, ids, aud, labels = _data(S)
    dims = LlamaDims(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH, vocab_size=V, mm_hidden_size=MM)
    eng = HipLlamaEngine(dims, "cuda", 2, max_seq, precision="bf16")
    eng.load_state_dict(w0 if w is None else w)
    segs = [(b, int((ids[b] == V - 2).nonzero()[0, 0]), aud[b].cuda()) for b in range(ids.shape[0])]
    return eng, segs


@functools.lru_cache(maxsize=None)
def _adapters(r, b_std=0.02):
    """bf16-representable adapter factors under peft names; B non-zero (at B = 0 dA is identically zero and shows nothing)."""
    from llark_amd.m2t import lora as LO
    cfg = LO.LoraConfig(r=r, alpha=16)
    ad = LO.init_adapters(cfg, H, I, LAYERS, seed=3)
    g = torch.Generator().manual_seed(11)
    for k in ad:
        ad[k] = _bf(torch.randn(ad[k].shape, generator=g) * b_std) if ".lora_B." in k else _bf(ad[k])
    return cfg, ad


TOKS = (V - 2, V - 1)


def _trainer(S, r=None, adapters=None, **kw):
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    eng, segs = _engine(S)
    if r is None:
        return HipLlamaTrainer(eng, embed_grad_tokens=TOKS, freeze_backbone=True, **kw), eng, segs
    cfg, ad = _adapters(r)
    tr = HipLlamaTrainer(eng, embed_grad_tokens=TOKS, lora=cfg, **kw)
    tr.set_adapters(ad if adapters is None else adapters)
    return tr, eng, segs


@functools.lru_cache(maxsize=None)
def _oracle(S, r):
    """(loss, gradients) of torch autograd over the oracle with W_eff = W + s B A; r = None: the plain model, leaves = every weight."""
    from llark_amd.m2t import lora as LO
    from oracle import llama_ref as LR
    spec, w, ids, aud, labels = _data(S)
    wp = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    leaves = {}
    if r is not None:
        cfg, ad = _adapters(r)
        leaves = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
        for i in range(LAYERS):
            for mod in LO.TARGET_MODULES:
                wk = LO.hf_weight_key(i, mod)
                wp[wk] = w[wk] + cfg.scale * (leaves[LO.peft_key(i, mod, "B")] @ leaves[LO.peft_key(i, mod, "A")])
    out = LR.forward(wp, spec, ids, aud, labels=labels, act_dtype=torch.bfloat16, round_probs=True)
    out["loss"].backward()
    grads = {k: v.grad for k, v in leaves.items()}
    for k in ("model.embed_tokens.weight", "model.mm_projector.weight", "model.mm_projector.bias"):
        grads[k] = wp[k].grad
    return out["loss"].item(), grads


def _compare(got, ref, spec_rows=TOKS):
    worst = {}
    for name, gh in got.items():
        r = ref[name]
        gh = gh.float().cpu()
        if name == "model.embed_tokens.weight":
            others = [i for i in range(V) if i not in spec_rows]
            assert gh[others].abs().max().item() == 0.0                       # every other embedding row gets exactly zero
            gh, r = gh[list(spec_rows)], r[list(spec_rows)]
        rel = ((gh - r).norm() / (r.norm() + 1e-30)).item()
        cos = torch.nn.functional.cosine_similarity(gh.flatten(), r.flatten(), dim=0).item()
        worst[name] = (rel, cos)
    top = sorted(worst.items(), key=lambda kv: -kv[1][0])[:4]
    print("worst grad rel errs:", [(k, f"{v[0]:.2e}", f"{v[1]:.5f}") for k, v in top])
    for name, (rel, cos) in worst.items():
        assert np.isfinite(rel) and rel <= 3e-2 and cos >= 0.999, f"{name}: rel {rel:.3e} cos {cos:.5f}"


@pytest.mark.parametrize("S", [20, 72])
@pytest.mark.parametrize("r", [8, 64])
def test_lora_gradients_match_autograd(S, r, monkeypatch):
    from llark_amd.m2t import lora as LO
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    spec, w, ids, aud, labels = _data(S)
    tr, eng, segs = _trainer(S, r)
    called, orig_dw = [], HipLlamaTrainer._dw
    monkeypatch.setattr(HipLlamaTrainer, "_dw", lambda self, dy, x, grad, name: (called.append(name), orig_dw(self, dy, x, grad, name))[1])
    from llark_amd import ops
    launches = {nm: 0 for nm in ("gemm16_fragw_rope_qkv_train", "gemm16_fragw_swiglu_train", "rope_split_heads", "swiglu_fwd", "swiglu_bwd",
                                 "attn_backward_fused", "attn_backward")}
    for nm in launches:
        def counted(*a, _nm=nm, _fn=getattr(ops, nm), **kw):
            launches[_nm] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, nm, counted)
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
    assert called == ["proj_w"]                                               # no dW product for a frozen matrix
    if S == 72:             # 144 rows: the adapters ride in the twins' extra K columns and every fused epilogue of the full step is kept
        assert launches == dict(gemm16_fragw_rope_qkv_train=LAYERS, gemm16_fragw_swiglu_train=2 * LAYERS, rope_split_heads=0, swiglu_fwd=0,
                                swiglu_bwd=0, attn_backward_fused=LAYERS, attn_backward=0), launches
    else:                   # 40 rows, below FRAG_MIN_ROWS: no twins, separate low-rank products around the base products
        assert launches == dict(gemm16_fragw_rope_qkv_train=0, gemm16_fragw_swiglu_train=0, rope_split_heads=LAYERS, swiglu_fwd=LAYERS,
                                swiglu_bwd=LAYERS, attn_backward_fused=0, attn_backward=LAYERS), launches
    ref_loss, ref = _oracle(S, r)
    print(f"loss {loss:.6f} ref {ref_loss:.6f}")
    assert abs(loss - ref_loss) <= 5e-3 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    got = tr.export_grads_hf()
    want = {LO.peft_key(i, m, ab) for i in range(LAYERS) for m in LO.TARGET_MODULES for ab in "AB"}
    want |= {"model.embed_tokens.weight", "model.mm_projector.weight", "model.mm_projector.bias"}
    assert set(got) == want                                                   # nothing for a frozen tensor
    assert got[LO.peft_key(0, "q_proj", "A")].shape == (r, H) and got[LO.peft_key(1, "down_proj", "B")].shape == (H, r)
    _compare(got, ref)
    for name, p in tr.params:                                                 # the rank padding takes no gradient
        if ".lora_" in name:
            assert tr.grads[name][:, r:].abs().max().item() == 0.0 if r < tr.lora.rp else True


def test_zero_b_gives_the_frozen_models_loss_and_no_gradient_for_a():
    from llark_amd.m2t import lora as LO
    S = 72
    spec, w, ids, aud, labels = _data(S)
    cfg = LO.LoraConfig(r=8)
    tr, eng, segs = _trainer(S, 8, adapters=LO.init_adapters(cfg, H, I, LAYERS, seed=1))
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
    ref_loss, _ = _oracle(S, None)
    assert abs(loss - ref_loss) <= 5e-3 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    trf, _, segs_f = _trainer(S)
    loss_f = trf.forward_backward(ids.cuda(), segs_f, labels.cuda()).item()
    assert abs(loss - loss_f) <= 5e-3 * max(1.0, abs(loss_f))
    g = tr.export_grads_hf()
    for k, v in g.items():
        if ".lora_A." in k:
            assert v.abs().max().item() == 0.0, k
        elif ".lora_B." in k:
            assert v.abs().max().item() > 0.0, k


def _operands_from_masters(tr):
    """The bf16 operands of every adapter group built explicitly with torch from the fp32 masters."""
    out = {}
    params, rp, s = dict(tr.params), tr.lora.rp, tr.lora.scale
    for key, g in tr._lora_groups.items():
        w = len(g.members) * rp
        a_stack = torch.zeros((w, g.k), dtype=torch.bfloat16, device="cuda")
        sb_diag = torch.zeros((g.ngrp, w), dtype=torch.bfloat16, device="cuda")
        for j, (mod, row0, blk, n) in enumerate(g.members):
            at, b = params[f"layers.{g.layer}.{mod}.lora_At"], params[f"layers.{g.layer}.{mod}.lora_B"]
            a_stack[j * rp: (j + 1) * rp] = at.t().bfloat16()
            rmap = torch.tensor([row0 + (i // 32) * blk + i % 32 for i in range(n)], device="cuda")
            sb_diag[rmap, j * rp: (j + 1) * rp] = (b * s).bfloat16()
        out[key] = dict(a_stack=a_stack, a_cat=a_stack.t().contiguous(), sb_diag=sb_diag, sb_t=sb_diag.t().contiguous())
    return out


_AUG = {"wqkv": ("qkv", 0), "wgu": ("gu", 0), "wo": ("o", 1), "wdown": ("down", 1)}


def _frozen_chunks(twin, nrows, kbase, kp):
    """The chunks of a fragment-major [nrows][kp] twin that hold its first kbase K columns (1-KiB chunks [32-row tile][16-wide k step])."""
    return twin.view(nrows // 32, kp // 16, 512)[:, : kbase // 16]


def _check_twins(tr, before=None):
    """Every twin equals ops.pack_weight16_frag of the operand built explicitly from W and the fp32 masters: [W | sB] (q|k|v in
    rope_qkv_row_order, gate|up) and W^T for the forward-augmented pair, W and [W^T | A^T] for o_proj / down_proj, whose dX product
    carries the adapter (the two-launch form).  ``before``: clones of the twins taken earlier; the frozen chunks still hold those bits."""
    from llark_amd import ops
    want = _operands_from_masters(tr)
    order = ops.rope_qkv_row_order(NH, H // NH).cuda()
    assert len(tr.twins) == 4 * LAYERS
    for name, (a, b, rope_rows) in tr.twins.items():
        _, layer, nm = name.split(".")
        gname, slot = _AUG[nm]
        ops_g = want[(int(layer), gname)]
        w = tr._matrices[name]
        n, k = w.shape
        width = ops_g["sb_diag"].shape[1]
        assert rope_rows == (2 * H if nm == "wqkv" else 0), name
        fwd = torch.cat((w, ops_g["sb_diag"]), dim=1) if slot == 0 else w
        if rope_rows:
            fwd = fwd.index_select(0, order)
        wt = ops.transposed16(w)
        bwd = torch.cat((wt, ops_g["a_cat"]), dim=1) if slot == 1 else wt
        assert torch.equal(a, ops.pack_weight16_frag(fwd.contiguous(), n)), name
        assert torch.equal(b, ops.pack_weight16_frag(bwd.contiguous(), k)), name
        # the frozen chunks are the pack of the base alone ...
        base_f = ops.pack_weight16_frag(w.index_select(0, order) if rope_rows else w, n)
        base_b = ops.pack_weight16_frag(wt, k)
        assert torch.equal(_frozen_chunks(a, n, k, fwd.shape[1]), base_f.view(n // 32, k // 16, 512)), name
        assert torch.equal(_frozen_chunks(b, k, n, bwd.shape[1]), base_b.view(k // 32, n // 16, 512)), name
        if before is not None:                                                # ... and bit-equal to what they were
            a0, b0 = before[name]
            assert a0.shape == a.shape and b0.shape == b.shape
            assert torch.equal(_frozen_chunks(a, n, k, fwd.shape[1]), _frozen_chunks(a0, n, k, fwd.shape[1])), name
            assert torch.equal(_frozen_chunks(b, k, n, bwd.shape[1]), _frozen_chunks(b0, k, n, bwd.shape[1])), name
            if (a if slot == 0 else b).numel() > n * k:
                assert not torch.equal(a if slot == 0 else b, a0 if slot == 0 else b0), name     # the tail did change


def test_refresh_rewrites_only_the_tails_of_the_augmented_twins():
    """Built with B = 0, then given known masters: each augmented twin is the fresh pack of the explicit [W | sB] / [W^T | A^T], q|k|v in
    the fused-RoPE row order, and the frozen chunks are bit-equal to what they were."""
    from llark_amd.m2t import lora as LO
    tr, eng, segs = _trainer(72, 8, adapters=LO.init_adapters(LO.LoraConfig(r=8), H, I, LAYERS, seed=1))
    _check_twins(tr)
    before = {n: (a.clone(), b.clone()) for n, (a, b, _) in tr.twins.items()}
    tr.set_adapters(_adapters(8)[1])
    _check_twins(tr, before)
    # a reload from outside re-packs everything into the same buffers
    ptrs = {n: (a.data_ptr(), b.data_ptr()) for n, (a, b, _) in tr.twins.items()}
    tr.refresh_derived()
    _check_twins(tr)
    assert ptrs == {n: (a.data_ptr(), b.data_ptr()) for n, (a, b, _) in tr.twins.items()}


def test_three_optimizer_steps_leave_the_base_bit_identical_and_the_operands_current():
    from llark_amd import ops
    S = 72
    spec, w, ids, aud, labels = _data(S)
    from llark_amd.m2t import lora as LO
    cfg = LO.LoraConfig(r=8)
    tr, eng, segs = _trainer(S, 8, adapters=LO.init_adapters(cfg, H, I, LAYERS, seed=1), lr=1e-2)
    frozen_names = [k for k in eng.state_dict_hf() if "mm_projector" not in k and "embed_tokens" not in k]
    before = {k: eng.state_dict_hf()[k].clone() for k in frozen_names}
    emb_before = eng.embed.clone()
    twins_before = {n: (a.clone(), b.clone()) for n, (a, b, _) in tr.twins.items()}
    assert len(tr.twins) == 4 * LAYERS
    losses = []
    for _ in range(3):
        losses.append(tr.forward_backward(ids.cuda(), segs, labels.cuda()).item())
        tr.step(max_grad_norm=1.0)
    losses.append(tr.forward_backward(ids.cuda(), segs, labels.cuda()).item())
    assert losses[-1] < losses[0], losses
    now = eng.state_dict_hf()
    for k in frozen_names:
        assert torch.equal(now[k], before[k]), k
    others = [i for i in range(V) if i not in TOKS]
    assert torch.equal(eng.embed[others], emb_before[others])
    _check_twins(tr, twins_before)                                            # the twins equal fresh packs of the current [W | sB]
    ad = tr.get_adapters()
    assert all(v.abs().max().item() > 0.0 for k, v in ad.items() if ".lora_B." in k)
    for name, p in tr.params:                                                 # padded columns: no update
        if ".lora_" in name:
            assert p[:, 8:].abs().max().item() == 0.0, name
    want = _operands_from_masters(tr)
    for key, g in tr._lora_groups.items():
        for nm, t in want[key].items():
            assert torch.equal(getattr(g, nm), t), (key, nm)


def test_parameter_table_covers_the_trainable_tensors_only():
    tr, eng, _ = _trainer(20, 8)
    rp = 64
    per_layer = sum((k + n) * rp for n, k in ((H, H),) * 4 + ((I, H),) * 2 + ((H, I),))
    small = eng.embed.numel() + eng.proj_w.numel() + eng.proj_b.numel()
    assert tr.flat_grad.numel() == tr.flat_m.numel() == tr.flat_v.numel() == LAYERS * per_layer + small
    assert sum(p.numel() for _, p in tr.params) == tr.flat_grad.numel()
    trf, engf, _ = _trainer(20)
    assert trf.flat_grad.numel() == small and [n for n, _ in trf.params] == ["embed", "proj_w", "proj_b"]
    from llark_amd.m2t.lora import LoraConfig
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    eng2, _ = _engine(20)
    sub = HipLlamaTrainer(eng2, embed_grad_tokens=TOKS, lora=LoraConfig(r=16, target_modules=("q_proj", "v_proj")))
    assert sub.flat_grad.numel() == LAYERS * 2 * (H + H) * rp + small


@pytest.mark.parametrize("S", [20, 72])
def test_frozen_backbone_gradients_match_autograd(S, monkeypatch):
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    spec, w, ids, aud, labels = _data(S)
    tr, eng, segs = _trainer(S)
    called, orig_dw = [], HipLlamaTrainer._dw
    monkeypatch.setattr(HipLlamaTrainer, "_dw", lambda self, dy, x, grad, name: (called.append(name), orig_dw(self, dy, x, grad, name))[1])
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
    ref_loss, ref = _oracle(S, None)
    assert abs(loss - ref_loss) <= 5e-3 * max(1.0, abs(ref_loss))
    assert called == ["proj_w"]                                               # no dW product for a frozen matrix
    got = tr.export_grads_hf()
    assert set(got) == {"model.embed_tokens.weight", "model.mm_projector.weight", "model.mm_projector.bias"}
    _compare(got, ref)
    before = {k: v.clone() for k, v in eng.state_dict_hf().items()}
    tr.step()
    now = eng.state_dict_hf()
    for k in before:
        assert torch.equal(now[k], before[k]) == ("mm_projector" not in k and "embed_tokens" not in k), k


def test_subset_of_targets_matches_autograd():
    """target_modules = (q_proj, v_proj, down_proj): a group with a member missing, groups without adapters beside augmented ones."""
    from llark_amd.m2t import lora as LO
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    from oracle import llama_ref as LR
    S, r = 72, 16
    spec, w, ids, aud, labels = _data(S)
    cfg = LO.LoraConfig(r=r, alpha=16, target_modules=("q_proj", "v_proj", "down_proj"))
    ad = LO.init_adapters(cfg, H, I, LAYERS, seed=4)
    g = torch.Generator().manual_seed(12)
    ad = {k: _bf(torch.randn(v.shape, generator=g) * 0.02) if ".lora_B." in k else _bf(v) for k, v in ad.items()}
    eng, segs = _engine(S)
    tr = HipLlamaTrainer(eng, embed_grad_tokens=TOKS, lora=cfg)
    tr.set_adapters(ad)
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
    wp = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
    for i in range(LAYERS):
        for mod in cfg.target_modules:
            wk = LO.hf_weight_key(i, mod)
            wp[wk] = w[wk] + cfg.scale * (leaves[LO.peft_key(i, mod, "B")] @ leaves[LO.peft_key(i, mod, "A")])
    out = LR.forward(wp, spec, ids, aud, labels=labels, act_dtype=torch.bfloat16, round_probs=True)
    out["loss"].backward()
    ref = {k: v.grad for k, v in leaves.items()}
    for k in ("model.embed_tokens.weight", "model.mm_projector.weight", "model.mm_projector.bias"):
        ref[k] = wp[k].grad
    assert abs(loss - out["loss"].item()) <= 5e-3 * max(1.0, abs(out["loss"].item()))
    got = tr.export_grads_hf()
    assert set(got) == set(ref)
    _compare(got, ref)


def test_checkpointing_and_loss_groups_give_the_plain_pass_gradients():
    """Gradient checkpointing re-runs the same kernels in the same order: adapter gradients bit for bit (llark_lora_dw joins its
    partial sums in a fixed order).  loss_groups = 2 over a batch of 4 = two separate micro-batches at scale 1/2: 2e-3 relative per
    tensor, the bar tests/test_train_gpu.py sets for the same comparison."""
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    S = 72
    spec, w, ids, aud, labels = _data(S)
    cfg, ad = _adapters(8)
    grads = []
    for ckpt in (False, True):
        tr, eng, segs = _trainer(S, 8, gradient_checkpointing=ckpt)
        loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
        grads.append((loss, {n: tr.grads[n].clone() for n, _ in tr.params}))
    assert grads[0][0] == grads[1][0]
    for n, a in grads[0][1].items():
        if ".lora_" in n or n == "proj_w":
            assert torch.equal(a, grads[1][1][n]), n
        else:
            assert torch.allclose(a, grads[1][1][n], rtol=1e-5, atol=1e-7), n
    # ---- loss_groups: B = 4 (the batch twice, the second copy with fewer label tokens)
    ids4, labels4, aud4 = torch.cat([ids, ids]), torch.cat([labels, labels]).clone(), torch.cat([aud, aud])
    labels4[2:, :40] = -100
    dims = LlamaDims(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=NH, vocab_size=V, mm_hidden_size=MM)
    eng = HipLlamaEngine(dims, "cuda", 4, 128, precision="bf16")
    eng.load_state_dict(w)
    segs = [(b, int((ids4[b] == V - 2).nonzero()[0, 0]), aud4[b].cuda()) for b in range(4)]
    tr = HipLlamaTrainer(eng, embed_grad_tokens=TOKS, lora=cfg)
    tr.set_adapters(ad)
    losses = []
    for gi in range(2):
        sl = slice(2 * gi, 2 * gi + 2)
        sg = [(b - 2 * gi, st, a) for (b, st, a) in segs[2 * gi: 2 * gi + 2]]
        losses.append(tr.forward_backward(ids4[sl].cuda(), sg, labels4[sl].cuda(), 0.5).item())
    sep = {k: v.float().clone() for k, v in tr.export_grads_hf().items()}
    tr.zero_grad()
    loss = tr.forward_backward(ids4.cuda(), segs, labels4.cuda(), 0.5, loss_groups=2).item()
    assert abs(loss - 0.5 * (losses[0] + losses[1])) <= 1e-5 * abs(loss)
    for name, gf in tr.export_grads_hf().items():
        rel = ((gf.float() - sep[name]).norm() / (sep[name].norm() + 1e-30)).item()
        assert np.isfinite(rel) and rel <= 2e-3, f"{name}: rel {rel:.3e}"


@pytest.mark.parametrize("S", [20, 72])
def test_clipping_norm_matches_torch_over_the_exported_gradients(S):
    spec, w, ids, aud, labels = _data(S)
    tr, eng, segs = _trainer(S, 8, lr=1e-3)
    tr.forward_backward(ids.cuda(), segs, labels.cuda(), last_micro_batch=True)
    exported = tr.export_grads_hf()
    ref = torch.sqrt(sum(v.double().pow(2).sum() for v in exported.values())).item()
    tr.step(max_grad_norm=0.05 * ref)
    assert abs(tr.last_grad_norm - ref) <= 1e-6 * ref, (tr.last_grad_norm, ref)


def test_checkpoint_round_trip(tmp_path):
    from llark_amd.m2t import checkpoint as CK
    from llark_amd.m2t import lora as LO
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    S = 20
    spec, w, ids, aud, labels = _data(S)
    cfg = LO.LoraConfig(r=8)
    out = str(tmp_path / "run")
    tr, eng, segs = _trainer(S, 8, adapters=LO.init_adapters(cfg, H, I, LAYERS, seed=0), lr=2e-3)
    for step in range(3):
        tr.forward_backward(ids.cuda(), segs, labels.cuda())
        tr.step()
        if step == 1:
            CK.save_checkpoint(tr, out, save_total_limit=1)
    final = tr.get_adapters()
    final_proj = eng.proj_w.float().clone()
    folder = os.path.join(out, "checkpoint-2")
    assert sorted(os.listdir(folder)) == ["adapter_config.json", "adapter_model.bin", "non_lora_trainables.bin", "trainer_state.pt"]
    saved = torch.load(os.path.join(folder, "adapter_model.bin"))
    assert set(saved) == {LO.peft_key(i, m, ab) for i in range(LAYERS) for m in LO.TARGET_MODULES for ab in "AB"}
    assert saved[LO.peft_key(0, "gate_proj", "A")].shape == (8, H) and saved[LO.peft_key(0, "gate_proj", "B")].shape == (I, 8)
    conf = json.load(open(os.path.join(folder, "adapter_config.json")))
    assert conf["r"] == 8 and conf["lora_alpha"] == 16 and conf["lora_dropout"] == 0.0 and conf["bias"] == "none"
    assert sorted(conf["target_modules"]) == sorted(LO.TARGET_MODULES)
    assert sorted(torch.load(os.path.join(folder, "non_lora_trainables.bin"))) == ["model.embed_tokens.weight", "model.mm_projector.bias",
                                                                                   "model.mm_projector.weight"]
    tr2, eng2, segs2 = _trainer(S, 8, adapters=LO.init_adapters(cfg, H, I, LAYERS, seed=5), lr=2e-3)     # other adapters: all restored
    assert CK.maybe_resume(tr2, out) == 2 and tr2.step_count == 2
    tr2.forward_backward(ids.cuda(), segs2, labels.cuda())
    tr2.step()
    got = tr2.get_adapters()
    for k in final:
        assert torch.equal(got[k], final[k]), k
    assert torch.equal(eng2.proj_w.float(), final_proj)
    # a checkpoint of another parameter table is refused
    eng3, _ = _engine(S)
    other = HipLlamaTrainer(eng3, embed_grad_tokens=TOKS, lora=LO.LoraConfig(r=8, target_modules=("q_proj",)))
    with pytest.raises(ValueError, match="different parameter table"):
        CK.load_checkpoint(other, folder)
    # frozen backbone without LoRA keeps the full layout
    trf, engf, segsf = _trainer(S)
    trf.forward_backward(ids.cuda(), segsf, labels.cuda())
    trf.step()
    CK.save_checkpoint(trf, str(tmp_path / "frozen"))
    assert os.path.exists(tmp_path / "frozen" / "checkpoint-1" / "pytorch_model.bin")


def test_merged_adapter_runs_through_the_inference_engine():
    from llark_amd.m2t import lora as LO
    from oracle import llama_ref as LR
    S = 72
    spec, w, ids, aud, labels = _data(S)
    cfg, ad = _adapters(8)
    tr, eng, segs = _trainer(S, 8)
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
    merged = LO.merge_into_state_dict(w, ad, cfg)
    eng2, segs2 = _engine(S, merged)
    logits = eng2.forward_tokens(ids.cuda(), segs2).float().cpu()
    lm = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100).item()
    assert abs(lm - loss) <= 5e-3 * max(1.0, abs(loss)), (lm, loss)


def test_train_cli_end_to_end_with_lora(tmp_path):
    """`python -m llark_amd.m2t.train --lora_enable True --lora_r 8` on a tiny HF-format checkpoint + tokenizer and synthetic shards
    (the set-up of tests/test_train_gpu.py::test_train_cli_end_to_end): adapters are written, no full model, a second call resumes;
    the saved adapter loads into the wrapped model for inference."""
    import io
    import tarfile
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from llark_amd.m2t import checkpoint as CK
    from llark_amd.m2t import lora as LO
    from llark_amd.m2t import train as T
    from llark_amd.m2t.llamav2 import WrappedLlamav2Config, WrappedLlamav2ForCausalLM
    from llark_amd.m2t.prompting import DEFAULT_CONVERSATION_HEADER
    words = sorted(set((DEFAULT_CONVERSATION_HEADER + " ### Human: Assistant: what is the genre ? it is jazz rock piano . <audio>").split()))
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    for wd in words:
        vocab.setdefault(wd, len(vocab))
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    ckpt = tmp_path / "ckpt"
    fast = PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", bos_token="<s>", eos_token="</s>")
    fast.save_pretrained(str(ckpt))
    cfg = WrappedLlamav2Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                               vocab_size=len(vocab), max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    torch.manual_seed(0)
    WrappedLlamav2ForCausalLM(cfg).save_pretrained(str(ckpt))
    rng = np.random.default_rng(0)
    with tarfile.open(tmp_path / "s-000.tar", "w") as tf:
        for k in range(4):
            payload = json.dumps({"response": [{"question": "what is the genre ?", "answer": "it is jazz ."}]}).encode()
            info = tarfile.TarInfo(f"k{k}.json")
            info.size = len(payload)
            tf.addfile(info, io.BytesIO(payload))
            b = io.BytesIO()
            np.save(b, rng.standard_normal((3, 96)).astype(np.float32))
            info = tarfile.TarInfo(f"k{k}.audio_encoding.npy")
            info.size = len(b.getvalue())
            tf.addfile(info, io.BytesIO(b.getvalue()))
    out = tmp_path / "out"
    argv = ["--model_name_or_path", str(ckpt), "--train_data_path", str(tmp_path / "s-{000..000}.tar"), "--output_dir", str(out),
            "--mm_hidden_size", "96", "--mm_use_audio_start_end", "True", "--per_device_train_batch_size", "2",
            "--gradient_accumulation_steps", "2", "--learning_rate", "1e-3", "--max_steps", "3", "--model_max_length", "128",
            "--save_steps", "2", "--save_total_limit", "2", "--bf16", "True", "--report_to", "none",
            "--lora_enable", "True", "--lora_r", "8", "--lora_alpha", "16"]
    T.main(argv)
    assert [os.path.basename(p) for p in CK.list_checkpoints(str(out))] == ["checkpoint-2", "checkpoint-3"]
    last = out / "checkpoint-3"
    assert (last / "adapter_model.bin").exists() and (last / "adapter_config.json").exists() and (last / "non_lora_trainables.bin").exists()
    assert not (last / "pytorch_model.bin").exists()
    ad = torch.load(last / "adapter_model.bin")
    assert ad[LO.peft_key(1, "v_proj", "B")].shape == (256, 8) and ad[LO.peft_key(1, "v_proj", "B")].abs().max().item() > 0.0
    T.main([("4" if a == "3" else a) for a in argv])                     # --max_steps 4: resumes from checkpoint-3, one more step
    assert os.path.basename(CK.latest_checkpoint(str(out))) == "checkpoint-4"
    # the adapter merges into the base model for inference, from the checkpoint folder as it was written: non_lora_trainables carries the
    # embedding resized for the added audio tokens and the projector, neither of which the base model has yet
    model = WrappedLlamav2ForCausalLM.from_pretrained(str(ckpt), torch_dtype=torch.bfloat16)
    base_q = model.state_dict()["model.layers.1.self_attn.v_proj.weight"].float().clone()
    model.load_lora_adapter(str(out / "checkpoint-4"))
    extra = torch.load(out / "checkpoint-4" / "non_lora_trainables.bin")
    now = model.state_dict()
    for k, v in extra.items():
        assert torch.equal(now[k].float().cpu(), v.to(now[k].dtype).float().cpu()), k
    ad4 = torch.load(out / "checkpoint-4" / "adapter_model.bin")
    want = base_q + 2.0 * (ad4[LO.peft_key(1, "v_proj", "B")] @ ad4[LO.peft_key(1, "v_proj", "A")])
    got = model.state_dict()["model.layers.1.self_attn.v_proj.weight"].float()
    assert torch.allclose(got, want.bfloat16().float(), rtol=0, atol=2 ** -8 * want.abs().max().item())
