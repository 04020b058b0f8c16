"""GPU: weights loaded IN PLACE into a live trainer or inference engine give what a fresh build on those weights gives, and the
shifted cross-entropy every training gradient starts from holds against float64 at the recipe's vocabulary.

The training step and the inference engine multiply by operands DERIVED from the weights (fragment-major W and W^T twins, the
q|k|v twin in the fused-RoPE row order, the frozen lm_head's W^T): a checkpoint copied into the row-major tensors must reach all
of them.  The resume cases therefore start the resumed run from OTHER weights than the checkpoint's, so that a stale derived
operand differs grossly instead of by one step's drift."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_train_gpu import _oracle_grads, _setup_long  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (environment, dx_direct_uses, gradient_checkpointing)
_CONFIGS = {
    "twins": ({}, None, False),                                   # the default: every product on the optimizer-maintained twins
    "derived_wT": ({"LLARK_TRAIN_TWINS": "0"}, 1, False),         # no twins: the per-step W^T / fragment-major caches (_derived)
    "checkpointing": ({}, None, True),                            # twins, each layer's forward re-run in the backward
}


def _trainer(eng, toks, monkeypatch, cfg):
    from llark_amd.m2t.train_engine import HipLlamaTrainer
    env, dx_uses, ckpt = _CONFIGS[cfg]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = HipLlamaTrainer(eng, lr=2e-3, embed_grad_tokens=toks, gradient_checkpointing=ckpt)
    if dx_uses is not None:
        tr.dx_direct_uses = dx_uses
    if cfg == "derived_wT":
        assert not tr.twins
    else:
        assert tr.twins and tr.rope_fused and tr.swiglu_fused
    return tr


def _check_derived_operands(tr, spec):
    """Every operand the trainer derives from its weights equals the one packed from the weights as they stand now."""
    from llark_amd import ops
    params = dict(tr.params)
    order = ops.rope_qkv_row_order(spec.num_attention_heads, 128).cuda()
    for name, (wfrag, wtfrag, rope_rows) in tr.twins.items():
        p = params[name]
        n, k = p.shape
        src = p.index_select(0, order) if rope_rows else p
        assert torch.equal(wfrag, ops.pack_weight16_frag(src, n)), f"{name}: W twin is stale"
        assert torch.equal(wtfrag, ops.pack_weight16_frag(ops.transposed16(p), k)), f"{name}: W^T twin is stale"
        if not rope_rows:
            assert p._llark_frag[0] is wfrag and torch.equal(p._llark_frag[0], ops.pack_weight16_frag(p, n)), name
    for name, p in params.items():                            # a weight without a twin carries no fragment-major copy of old values
        fr = getattr(p, "_llark_frag", None)
        if name not in tr.twins and fr is not None:
            assert torch.equal(fr[0], ops.pack_weight16_frag(p, fr[1])), f"{name}: attached fragment-major copy is stale"
    lm = tr.eng.lm_head
    wT = tr._frozen_wT.get(lm.data_ptr())
    if tr.twins:
        assert wT is not None and hasattr(lm, "_llark_frag")
    if wT is not None:
        assert torch.equal(lm._llark_frag[0], ops.pack_weight16_frag(lm, lm.shape[0])), "lm_head fragment-major copy is stale"
        assert torch.equal(wT, ops.transposed16(lm)), "lm_head W^T is stale"
        assert torch.equal(wT._llark_frag[0], ops.pack_weight16_frag(wT, wT.shape[0])), "lm_head W^T fragment-major copy is stale"


def _check_grads_vs_oracle(tr, loss, spec, w, ids, aud, labels):
    """The bars of test_twin_paths_gradients_match_autograd_and_survive_an_optimizer_step."""
    ref_loss, ref = _oracle_grads(spec, w, ids, aud, labels)
    assert abs(loss - ref_loss) <= 5e-3 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    for name, gh in tr.export_grads_hf().items():
        r = ref[name]
        gh = gh.float().cpu()
        if name == "model.embed_tokens.weight":
            rows = [spec.audio_start_token, spec.audio_end_token]
            gh, r = gh[rows], r[rows]
        rel = ((gh - r).norm() / (r.norm() + 1e-30)).item()
        cos = torch.nn.functional.cosine_similarity(gh.flatten(), r.flatten(), dim=0).item()
        assert np.isfinite(rel) and rel <= 3e-2 and cos >= 0.999, f"{name}: rel {rel:.3e} cos {cos:.5f}"


def _load_weights(folder):
    """The checkpoint's weights as the oracle's fp32 operands (bf16 matrices exactly, the fp32 norm gains and bias as stored)."""
    return {k: v.float() for k, v in torch.load(os.path.join(folder, "pytorch_model.bin")).items()}


@pytest.mark.parametrize("cfg", list(_CONFIGS))
def test_resume_at_twin_shapes_from_other_weights(tmp_path, monkeypatch, cfg):
    """2 steps (gradient clipping on), save, a 3rd step; then resume into an engine + trainer built from OTHER weights: every derived
    operand is the one packed from the loaded weights, the 3rd step's gradients match autograd on the checkpoint, and the weights after
    it equal the uninterrupted run's."""
    from llark_amd.m2t import checkpoint as CK
    spec, w, ids, aud, labels, eng, segs = _setup_long()
    toks = (spec.audio_start_token, spec.audio_end_token)
    tr = _trainer(eng, toks, monkeypatch, cfg)
    out = str(tmp_path / "run")
    for step in range(3):
        tr.forward_backward(ids.cuda(), segs, labels.cuda())
        tr.step(max_grad_norm=1.0)
        if step == 1:
            CK.save_checkpoint(tr, out, save_total_limit=1)
    final = {k: v.float().cpu().clone() for k, v in eng.state_dict_hf().items()}
    w_ck = _load_weights(os.path.join(out, "checkpoint-2"))
    _, w_other, _, _, _, eng2, segs2 = _setup_long(seed=1)
    assert not torch.equal(w_other["lm_head.weight"], w["lm_head.weight"])
    tr2 = _trainer(eng2, toks, monkeypatch, cfg)
    assert CK.maybe_resume(tr2, out) == 2 and tr2.step_count == 2
    for k, v in eng2.state_dict_hf().items():
        assert torch.equal(v.float().cpu(), w_ck[k]), k
    # (1) derived operands follow the loaded weights
    _check_derived_operands(tr2, spec)
    # (2) the 3rd step's loss and gradients against autograd on the checkpoint's weights
    loss = tr2.forward_backward(ids.cuda(), segs2, labels.cuda()).item()
    _check_grads_vs_oracle(tr2, loss, spec, w_ck, ids, aud, labels)
    # (3) after the 3rd step: the uninterrupted run's weights (the bar of test_checkpoint_resume_and_adapter_sidefile; the clip
    # coefficient comes from a sum of squares with atomic adds, so bit-equality is not promised)
    tr2.step(max_grad_norm=1.0)
    got = {k: v.float().cpu() for k, v in eng2.state_dict_hf().items()}
    same = [k for k in final if torch.equal(got[k], final[k])]
    print(f"{cfg}: {len(same)} of {len(final)} tensors bit-equal to the uninterrupted run")
    for k in final:
        assert torch.allclose(got[k], final[k], rtol=0, atol=2 ** -8 * max(1e-3, final[k].abs().max().item())), k


@pytest.mark.parametrize("cfg", list(_CONFIGS))
def test_checkpoint_into_a_live_trainer_equals_a_fresh_trainer(tmp_path, monkeypatch, cfg):
    """A trainer that has stepped past a checkpoint (twins rewritten, _wver > 0) and filled its per-step caches with one more
    micro-batch loads that older checkpoint: its next gradients are those of a fresh engine + trainer loaded from it."""
    from llark_amd.m2t import checkpoint as CK
    spec, w, ids, aud, labels, eng, segs = _setup_long()
    toks = (spec.audio_start_token, spec.audio_end_token)
    tr = _trainer(eng, toks, monkeypatch, cfg)
    out = str(tmp_path / "run")
    for step in range(3):
        tr.forward_backward(ids.cuda(), segs, labels.cuda())
        tr.step(max_grad_norm=1.0)
        if step == 0:
            CK.save_checkpoint(tr, out, save_total_limit=None)
    tr.forward_backward(ids.cuda(), segs, labels.cuda())
    tr.forward_backward(ids.cuda(), segs, labels.cuda(), loss_scale=0.5)   # second use since the step: per-step caches built
    assert tr._wver == 3
    folder = os.path.join(out, "checkpoint-1")
    assert CK.load_checkpoint(tr, folder) == 1
    _check_derived_operands(tr, spec)
    loss = tr.forward_backward(ids.cuda(), segs, labels.cuda()).item()
    _, _, _, _, _, eng_f, segs_f = _setup_long(seed=1)
    tr_f = _trainer(eng_f, toks, monkeypatch, cfg)
    assert CK.load_checkpoint(tr_f, folder) == 1
    loss_f = tr_f.forward_backward(ids.cuda(), segs_f, labels.cuda()).item()
    assert abs(loss - loss_f) <= 5e-3 * max(1.0, abs(loss_f)), (loss, loss_f)
    for name, prm in tr.params:
        a, b = tr.grads[name].float(), tr_f.grads[name].float()
        if prm.dim() == 2:                                       # same kernels on the same operands (cf. the twin-path test)
            assert torch.equal(a, b), name
        rel = ((a - b).norm() / (b.norm() + 1e-30)).item()
        assert rel <= 3e-2, f"{name}: rel {rel:.3e}"
    _check_grads_vs_oracle(tr, loss, spec, _load_weights(folder), ids, aud, labels)
    assert tr._wver > 3                                          # the load counts as a weight change: per-step caches start over


@pytest.mark.parametrize("precision", ["split", "bf16"])
def test_copy_weights_into_a_live_engine_equals_a_fresh_engine(precision):
    """An inference engine that has run a fragment-major prefill (>= 129 rows, fused-RoPE q|k|v twin) and captured its decode step takes
    other weights through copy_weights_into_engine: prefill logits and 8 greedy decode steps are bit-equal to a fresh engine's, and the
    captured decode graph is kept (every buffer it reads was rewritten in place)."""
    from llark_amd.m2t.checkpoint import copy_weights_into_engine
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    from oracle import llama_ref as LR
    spec = LR.LlamaSpec(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, vocab_size=320,
                        mm_hidden_size=96, audio_start_token=317, audio_end_token=318, audio_patch_token=319)
    dims = LlamaDims(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, vocab_size=320,
                     mm_hidden_size=96, rms_norm_eps=spec.rms_norm_eps)
    w_a, w_b = LR.make_weights(spec, seed=3, std=0.08), LR.make_weights(spec, seed=4, std=0.08)
    B, S = 3, 48
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, 300, (B, S), generator=g).cuda()

    def engine(w):
        eng = HipLlamaEngine(dims, "cuda", B, 128, precision=precision)
        eng.load_state_dict(w)
        eng.decode_graph, eng.fuse_prefill_rope = True, "1"
        return eng

    def run(eng):
        logits = eng.forward_tokens(ids).clone()
        assert all(L.wqkv_rope is not None for L in eng.layers), "the prefill did not take the fused-RoPE q|k|v twin"
        tok, steps = logits[:, -1:].argmax(-1), []
        for _ in range(8):
            lg = eng.forward_tokens(tok, (), pos0=eng.cur_len).clone()
            steps.append(lg)
            tok = lg[:, -1:].argmax(-1)
        return logits, torch.stack(steps)

    live = engine(w_a)
    old = run(live)
    graph = live._dec[B]["graph"]
    assert graph is not None, "the decode step was not captured"
    copy_weights_into_engine(live, w_b)
    got = run(live)
    assert live._dec[B]["graph"] is graph
    ref = run(engine(w_b))
    assert not torch.equal(old[0], ref[0])
    assert torch.equal(got[0], ref[0]), f"prefill logits differ: max |d| {(got[0] - ref[0]).abs().max().item():.3e}"
    assert torch.equal(got[1].argmax(-1), ref[1].argmax(-1)), "greedy tokens differ"
    assert torch.equal(got[1], ref[1]), f"decode logits differ: max |d| {(got[1] - ref[1]).abs().max().item():.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# cross-entropy forward + backward at the recipe's vocabulary (32004: 4 past a multiple of 64, dlogits pitch 32064)
# ---------------------------------------------------------------------------------------------------------------------------------
_V, _LDD, _SCALE = 32004, 32064, 0.25


def _ce_ref(logits, labels, scale, ignore_index=-100):
    """float64: mean shifted NLL over the counted rows and (softmax - onehot) * scale / count on them, zero elsewhere."""
    B, S, V = logits.shape
    lg = logits.double()[:, :-1].reshape(-1, V)
    tgt = labels[:, 1:].reshape(-1)
    counted = (tgt != ignore_index) & (tgt >= 0) & (tgt < V)
    n = int(counted.sum())
    lsm = torch.log_softmax(lg, dim=-1)
    rows = counted.nonzero().reshape(-1)
    loss = -lsm[rows, tgt[rows]].sum() / n if n else torch.tensor(float("nan"), dtype=torch.float64)
    grad = torch.zeros((B, S, V), dtype=torch.float64)
    if n:
        gr = lsm[rows].exp()
        gr[torch.arange(rows.numel()), tgt[rows]] -= 1.0
        gv = grad[:, :-1].reshape(-1, V)
        gv[rows] = gr * (scale / n)
        grad[:, :-1] = gv.view(B, S - 1, V)
    return float(loss), grad.reshape(B * S, V), n, counted


def _ce_run(logits, labels):
    from llark_amd import ops
    B, S, _ = logits.shape
    dl = torch.full((B * S, _LDD), 7.0, dtype=torch.bfloat16, device="cuda")      # every element must be written
    loss = ops.cross_entropy_fwd_bwd(logits.cuda(), labels.cuda(), dl, _SCALE)
    torch.cuda.synchronize()
    return float(loss.item()), dl.float().cpu()


def _ce_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    B, S = 2, 72
    logits = torch.randn(B, S, _V, generator=g) * 3.0
    labels = torch.randint(0, _V, (B, S), generator=g)
    return logits, labels


def test_cross_entropy_at_the_recipe_vocabulary_vs_float64():
    """Ignored rows, targets 0 and V - 1, a row whose target dominates by 60 (loss ~ 0), a row of +-80 logits (most exponentials
    underflow), labels outside [0, V) (not counted): loss to 1e-5, dlogits to bf16 rounding, pad columns and ignored rows exactly 0."""
    logits, labels = _ce_inputs(11)
    B, S, V = logits.shape
    labels[:, :5] = -100                                            # rows 0..3 of each sequence ignored
    labels[0, 10], labels[1, 20] = 0, V - 1                         # first and last vocabulary entry
    labels[0, 30], labels[1, 31] = V, -7                            # outside [0, V): not counted
    dom = (1, 40)                                                   # row (1, 40) predicts labels[1, 41]
    logits[dom[0], dom[1], labels[1, 41]] = logits[dom[0], dom[1]].max() + 60.0
    big = (0, 50)
    sign = torch.where(torch.randn(V, generator=torch.Generator().manual_seed(12)) > 0, 80.0, -80.0)
    logits[big[0], big[1]] = sign
    ref_loss, ref_g, n, counted = _ce_ref(logits, labels, _SCALE)
    assert 0 < n < B * (S - 1) and not counted[29] and not counted[S - 1 + 30]
    loss, got = _ce_run(logits, labels)
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert (got[:, V:] == 0).all(), "pad columns V .. ldd-1 are not zero"
    g = got[:, :V].double()
    tol = 2.0 ** -8 * ref_g.abs() + 2.0 ** -24 * _SCALE / n
    err = (g - ref_g).abs()
    bad = err > tol
    assert not bad.any(), (f"{int(bad.sum())} dlogits out of tolerance; worst row {int(bad.nonzero()[0, 0])}: "
                           f"max err {err.max().item():.3e}")
    row_of = lambda b, s: b * S + s                                  # noqa: E731
    skipped = [row_of(b, s) for b in range(B) for s in range(S) if s == S - 1 or not counted[b * (S - 1) + s]]
    assert (got[skipped] == 0).all(), "ignored rows are not zero"
    assert torch.isfinite(g).all()
    assert ref_g[row_of(*dom)].abs().max().item() < 1e-20 and g[row_of(*dom)].abs().max().item() < 1e-20   # loss ~ 0 row


def test_cross_entropy_every_label_ignored():
    """No counted row: the mean is NaN (torch's 0 / 0) and every dlogits element, pad columns included, is 0."""
    logits, labels = _ce_inputs(13)
    labels[:] = -100
    ref_loss, _, n, _ = _ce_ref(logits, labels, _SCALE)
    assert n == 0 and np.isnan(ref_loss)
    loss, got = _ce_run(logits, labels)
    assert np.isnan(loss), loss
    assert (got == 0).all()


def test_cross_entropy_nan_logit_in_a_counted_row():
    """A NaN logit in a counted row makes the loss NaN, as torch reports it (a diverging run must not log a normal-looking loss); that
    row's gradient is NaN, and every other row keeps the gradient of the mean over ALL counted rows."""
    logits, labels = _ce_inputs(17)
    B, S, V = logits.shape
    labels[:, :3] = -100
    b, s = 1, 33
    logits[b, s, 1234] = float("nan")
    ref_loss, ref_g, n, counted = _ce_ref(logits, labels, _SCALE)
    assert counted[b * (S - 1) + s] and np.isnan(ref_loss)
    tl = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
    assert torch.isnan(tl)
    loss, got = _ce_run(logits, labels)
    assert np.isnan(loss), f"loss {loss} with a NaN logit in a counted row (torch: {tl.item()})"
    row = b * S + s
    assert torch.isnan(got[row, :V]).all() and (got[row, V:] == 0).all()
    others = [r for r in range(B * S) if r != row]
    g, rg = got[others, :V].double(), ref_g[others]
    err = (g - rg).abs()
    assert not (err > 2.0 ** -8 * rg.abs() + 2.0 ** -24 * _SCALE / n).any(), f"max err {err.max().item():.3e}"
    assert (got[others, V:] == 0).all()
