"""MPT training through ``train()`` and the CLI, and ``HipMptTrainer.forward_backward_packed``: a whole optimizer step of ragged
micro-batches as ONE row stream on the ALiBi variable-length attention kernels (llark_attn_*_varlen_alibi).

The packed step is held to torch autograd over the fp32 oracle (oracle/mpt_ref.py), called once per micro-batch on right-padded rows
with label -100 -- the loss is the mean of the micro-batch means -- under the bars of
tests/test_mpt_gpu.py::test_mpt_training_step_gradients_match_autograd: loss within 1e-2 max(1, ref), every tensor within relative
Frobenius error 5e-2 and cosine 0.995, tensors whose reference gradient is < 1e-4 of the largest small on the GPU too.  The shipped
per-micro-batch loop runs on the same examples under the same bars.  That the oracle's loss on a right-padded micro-batch equals its
loss on the unpadded rows (pad keys lie behind every real query; ALiBi's ``-(S - 1)`` shift is a constant of the row) is checked on
the CPU first.  Dimensions and helpers are those of tests/test_mpt_gpu.py; the clip values are that test's, for the reason given there.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_mpt_gpu import BASE, _engine

gpu = pytest.mark.gpu

V, MM, F = BASE["vocab_size"], BASE["mm_hidden_size"], 4
START, END, PATCH = 93, 94, 95
PAD_ID = 0
CASES = {"twins": ((72, 40, 23, 56), (2, 2)), "small": ((20, 13), (1, 1))}
CONFIGS = {"alibi": {}, "alibi+qk_ln+clip+bias+logit_scale": dict(qk_ln=True, clip_qkv=3.0, no_bias=False, alibi_bias_max=4, logit_scale=0.5)}


@functools.lru_cache(maxsize=None)
def _data(case, config):
    """weights + the examples of one optimizer step: 1-D ids / labels per example, one audio clip each"""
    from oracle import mpt_ref as MR
    lengths, groups = CASES[case]
    spec = MR.MptSpec(**BASE, audio_start_token=START, audio_end_token=END, audio_patch_token=PATCH, **CONFIGS[config])
    w = MR.make_weights(spec, seed=31, std=0.08)
    g = torch.Generator().manual_seed(6)
    ids, labels = [], []
    for b, n in enumerate(lengths):
        head = 1 + b % 2
        t = torch.tensor([1] + torch.randint(3, 90, (head,), generator=g).tolist() + [START] + [PATCH] * F + [END]
                         + torch.randint(3, 90, (n - F - 3 - head,), generator=g).tolist())
        assert t.shape == (n,)
        lab = t.clone()
        lab[:9] = -100
        ids.append(t)
        labels.append(lab)
    aud = torch.randn(len(lengths), F, MM, generator=g)
    return spec, w, ids, labels, aud, groups


def _micro_batches(case, config):
    """the step as the shipped loop sees it: per micro-batch (ids [B][S], labels, audio [B][F][MM]) right-padded to its longest example"""
    spec, w, ids, labels, aud, groups = _data(case, config)
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
    return int((t == START).nonzero()[0, 0])


def _trainer(case, config, weights=None, **kw):
    from llark_amd.m2t.mpt_train_engine import HipMptTrainer
    spec, w = _data(case, config)[:2]
    return HipMptTrainer(_engine(spec, w if weights is None else weights, "bf16", max_batch=2, max_seq=128), **kw)


def _run_packed(tr, case, config):
    spec, w, ids, labels, aud, groups = _data(case, config)
    segs = [(b, _start(t), aud[b].cuda()) for b, t in enumerate(ids)]
    return tr.forward_backward_packed(ids, segs, labels, groups, pad_id=PAD_ID).item()


def _run_loop(tr, case, config):
    """the shipped loop: one right-padded forward_backward per micro-batch, gradients accumulated"""
    mbs = _micro_batches(case, config)
    loss = 0.0
    for mi, ml, ma in mbs:
        segs = [(b, _start(mi[b]), ma[b].cuda()) for b in range(mi.shape[0])]
        loss += tr.forward_backward(mi.cuda(), segs, ml.cuda(), 1.0 / len(mbs)).item() / len(mbs)
    return loss


@functools.lru_cache(maxsize=None)
def _oracle(case, config):
    """loss and gradients of the step by torch autograd: the oracle once per right-padded micro-batch, the mean of the micro-batch means"""
    from oracle import mpt_ref as MR
    spec, w = _data(case, config)[:2]
    wp = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    mbs = _micro_batches(case, config)
    total = sum(MR.forward(wp, spec, mi, ma, labels=ml)["loss"] for mi, ml, ma in mbs) / len(mbs)
    total.backward()
    return total.item(), {k: v.grad for k, v in wp.items()}


def _check(tag, loss, got, ref_loss, ref):
    """the bars of test_mpt_training_step_gradients_match_autograd"""
    assert abs(loss - ref_loss) <= 1e-2 * max(1.0, ref_loss), (tag, loss, ref_loss)
    biggest = max(g.norm().item() for g in ref.values() if g is not None)
    worst = {}
    for name, gg in got.items():
        a, b_ = gg.float().cpu().reshape(-1), ref[name].reshape(-1)
        if b_.norm().item() < 1e-4 * biggest:        # e.g. k_ln.bias: a constant added to every key cancels in the softmax -> exact 0
            assert a.norm().item() < 1e-2 * biggest, f"{tag} {name}: reference gradient ~0 but got norm {a.norm().item():.3e}"
            continue
        rel = ((a - b_).norm() / (b_.norm() + 1e-12)).item()
        cos = (torch.dot(a, b_) / (a.norm() * b_.norm() + 1e-20)).item()
        worst[name] = (rel, cos)
        assert rel <= 5e-2 and cos >= 0.995, f"{tag} {name}: rel {rel:.3e} cos {cos:.5f}"
    print(f"{tag}: loss {loss:.6f} (ref {ref_loss:.6f}); worst grad rel errs:", sorted(((v[0], k) for k, v in worst.items()), reverse=True)[:3])


def test_oracle_loss_on_a_right_padded_micro_batch_equals_the_unpadded_rows():
    """CPU: what makes the per-micro-batch oracle on padded rows a reference for the packed stream -- the pad rows (label -100, behind
    every real query in the causal order) change no example's loss, with ALiBi's bias taken from the padded length"""
    from oracle import mpt_ref as MR
    for config in CONFIGS:
        spec, w, ids, labels, aud, groups = _data("twins", config)
        b0 = 0
        for (mi, ml, ma), gsize in zip(_micro_batches("twins", config), groups):
            padded = MR.forward(w, spec, mi, ma, labels=ml)["loss"].item()
            num, den = 0.0, 0
            for j in range(gsize):
                t, lab = ids[b0 + j], labels[b0 + j]
                n_tgt = int((lab[1:] != -100).sum())
                num += MR.forward(w, spec, t[None], aud[b0 + j][None], labels=lab[None])["loss"].item() * n_tgt
                den += n_tgt
            assert abs(padded - num / den) <= 1e-5 * max(1.0, abs(padded)), (config, padded, num / den)
            b0 += gsize


@gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("case", list(CASES))
def test_mpt_packed_step_matches_autograd_and_the_shipped_loop(case, config):
    ref_loss, ref = _oracle(case, config)
    tr = _trainer(case, config)
    loss = _run_packed(tr, case, config)
    packed = {k: v.clone() for k, v in tr.export_grads_ref().items()}
    assert "transformer.wte.weight" not in packed and set(packed) == set(ref) - {"transformer.wte.weight"}
    _check(f"packed {case} {config}", loss, packed, ref_loss, ref)
    tr.zero_grad()
    loss_l = _run_loop(tr, case, config)
    loop = tr.export_grads_ref()
    _check(f"loop {case} {config}", loss_l, loop, ref_loss, ref)
    biggest = max(g.norm().item() for g in ref.values())
    diff = max(((packed[k].float() - loop[k].float()).norm() / loop[k].float().norm()).item() for k in loop
               if ref[k].norm().item() >= 1e-4 * biggest)                       # (the tensors _check compares by relative error)
    print(f"packed vs loop {case} {config}: loss {loss:.6f} / {loss_l:.6f}, largest relative gradient difference {diff:.3e}")


@gpu
def test_mpt_packed_step_with_train_wte_accumulates_both_uses():
    """``train_wte=True``: the tied table gets the gather rows' gradient and the logits product's, summed, in the packed stream too"""
    case, config = "twins", "alibi+qk_ln+clip+bias+logit_scale"
    ref_loss, ref = _oracle(case, config)
    tr = _trainer(case, config, train_wte=True)
    loss = _run_packed(tr, case, config)
    got = tr.export_grads_ref()
    assert set(got) == set(ref)
    _check("packed train_wte", loss, got, ref_loss, ref)


@gpu
def test_mpt_packed_step_refuses_what_the_caches_cannot_hold():
    tr = _trainer("small", "alibi")
    long = [torch.randint(3, 90, (120,)) for _ in range(3)]                   # 360 rows > max_batch * smax = 2 * 128
    with pytest.raises(ValueError, match="s_total = 360.*max_batch \\* smax"):
        tr.forward_backward_packed(long, [], [t.clone() for t in long], (3,))


def _audio_cfg(spec):
    from llark_amd.m2t import AudioEncoderConfig
    ac = AudioEncoderConfig()
    ac.audio_start_token, ac.audio_end_token, ac.audio_patch_token = spec.audio_start_token, spec.audio_end_token, spec.audio_patch_token
    return ac


@gpu
def test_train_loop_drives_the_mpt_trainer_with_and_without_pack_sequences():
    """``train()`` on a ``HipMptEngine``: three optimizer steps over the same ragged micro-batches with ``pack_sequences`` and without;
    the logged losses agree within the bar tests/test_train_packed_gpu.py uses for the same comparison on Llama, 5e-3 max(1, |loss|).
    ``fuse_accumulation`` runs the per-micro-batch loop and says so once."""
    from llark_amd.m2t.train import TrainConfig, train
    config = "alibi+qk_ln+clip+bias+logit_scale"
    spec, w = _data("twins", config)[:2]
    ac = _audio_cfg(spec)
    stream = [dict(input_ids=mi, labels=ml, attention_mask=mi.ne(PAD_ID), audio_encodings=ma) for mi, ml, ma in _micro_batches("twins", config)] * 3

    def run(records=None, **kw):
        e = _engine(spec, w, "bf16", max_batch=4 if kw.get("pack_sequences") else 2, max_seq=128)
        return train(e, stream, ac, TrainConfig(learning_rate=2e-3, max_steps=20, gradient_accumulation_steps=2, **kw), world=1,
                     log=records.append if records is not None else None)

    base, packed = run(), run(pack_sequences=True)
    print("mpt train loop losses:", base, "packed:", packed)
    assert len(base) == len(packed) == 3
    assert all(abs(a - b) <= 5e-3 * max(1.0, abs(a)) for a, b in zip(base, packed)), (base, packed)
    assert packed[-1] < packed[0]
    records = []
    fused = run(records, fuse_accumulation=True)
    assert all(abs(a - b) <= 5e-3 * max(1.0, abs(a)) for a, b in zip(base, fused)), (base, fused)
    notes = [r for r in records if "note" in r]
    assert len(notes) == 1 and "--fuse_accumulation" in notes[0]["note"] and [r["step"] for r in records if "step" in r] == [1, 2, 3]
    for flag in ("freeze_backbone", "lora_enable", "gradient_checkpointing"):
        with pytest.raises(NotImplementedError, match=f"--{flag}"):
            run(**{flag: True})


def _steps(tr, case, config, n):
    for _ in range(n):
        _run_packed(tr, case, config)
        tr.step(max_grad_norm=1.0)


def _state(tr):
    sd = {k: v.detach().clone() for k, v in tr.eng.state_dict().items()}
    sd["exp_avg"], sd["exp_avg_sq"] = tr.flat_m.clone(), tr.flat_v.clone()
    return sd


@gpu
def test_mpt_checkpoint_round_trip(tmp_path):
    """Two packed steps, save, a fresh engine holding OTHER weights, resume, one more step: the same weights and AdamW moments as the
    uninterrupted three steps.  The uninterrupted run is first run twice: where it repeats itself bit for bit the resumed run must be
    bit-equal too (the checkpoint holds the bf16 weights, the fp32 LayerNorm tensors and the fp32 moments exactly); where it does not
    (fp32 sums accumulated with atomics in the LayerNorm / bias gradients) every tensor must be within the gradient bars of this file
    (relative Frobenius error 5e-2, cosine 0.995).  On the MI355X the uninterrupted run did NOT repeat itself bit for bit."""
    from llark_amd.m2t import checkpoint as CK
    from oracle import mpt_ref as MR
    case, config = "small", "alibi+qk_ln+clip+bias+logit_scale"
    spec = _data(case, config)[0]
    runs = []
    for _ in range(2):
        tr = _trainer(case, config, lr=2e-3)
        _steps(tr, case, config, 3)
        runs.append(_state(tr))
    repeatable = all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    tr = _trainer(case, config, lr=2e-3)
    _steps(tr, case, config, 2)
    out = str(tmp_path / "out")
    folder = CK.save_checkpoint(tr, out)
    assert os.path.basename(folder) == "checkpoint-2"
    saved = torch.load(os.path.join(folder, "pytorch_model.bin"))
    assert set(saved) == set(MR.make_weights(spec, seed=1)) and saved["transformer.wte.weight"].dtype == torch.bfloat16
    side = torch.load(os.path.join(out, "mm_projector", "checkpoint-2.bin"))
    assert sorted(side) == ["transformer.mm_projector.bias", "transformer.mm_projector.weight"]
    tr2 = _trainer(case, config, weights=MR.make_weights(spec, seed=77, std=0.05), lr=2e-3)
    assert CK.maybe_resume(tr2, out) == 2 and tr2.step_count == 2
    for k, v in tr.eng.state_dict().items():
        assert torch.equal(tr2.eng.state_dict()[k], v), f"{k}: not restored"
    assert torch.equal(tr2.flat_m, tr.flat_m) and torch.equal(tr2.flat_v, tr.flat_v)          # the restore itself is exact either way
    _steps(tr2, case, config, 1)
    got = _state(tr2)
    print("mpt checkpoint round trip: the uninterrupted run repeats itself bit for bit:", repeatable)
    for k, want in runs[0].items():
        if repeatable:
            assert torch.equal(got[k], want), f"{k}: the resumed run differs from the uninterrupted one"
        else:
            a, b_ = got[k].double().reshape(-1), want.double().reshape(-1)
            rel, cos = ((a - b_).norm() / (b_.norm() + 1e-30)).item(), (torch.dot(a, b_) / (a.norm() * b_.norm() + 1e-30)).item()
            assert rel <= 5e-2 and cos >= 0.995, f"{k}: resumed run rel {rel:.3e} cos {cos:.5f} from the uninterrupted one"
    other = _trainer(case, config, train_wte=True)
    with pytest.raises(ValueError, match="different parameter table"):
        CK.load_checkpoint(other, folder)


@gpu
def test_train_cli_end_to_end_with_mpt(tmp_path):
    """``python -m llark_amd.m2t.train --model_name_or_path <.../mpt-tiny> --pack_sequences True`` on a tiny MPT folder + tokenizer and
    synthetic shards (the set-up of tests/test_lora_train_gpu.py::test_train_cli_end_to_end_with_lora): the name selects the MPT
    backbone, checkpoints are written under the reference's MPT names, a second call resumes, and the checkpoint folder opens with
    ``WrappedMPTForCausalLM.from_pretrained`` and generates."""
    import io
    import tarfile
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import AutoTokenizer, PreTrainedTokenizerFast
    from llark_amd.m2t import checkpoint as CK
    from llark_amd.m2t import train as T
    from llark_amd.m2t.mpt import WrappedMPTConfig, WrappedMPTForCausalLM
    from llark_amd.m2t.prompting import DEFAULT_CONVERSATION_HEADER
    words = sorted(set((DEFAULT_CONVERSATION_HEADER + " ### Human: Assistant: what is the genre ? it is jazz rock piano . <audio>").split()))
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    for wd in words:
        vocab.setdefault(wd, len(vocab))
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    ckpt = tmp_path / "mpt-tiny"
    assert T.backbone_of(str(ckpt)) == "mpt"
    fast = PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", bos_token="<s>", eos_token="</s>")
    fast.save_pretrained(str(ckpt))
    cfg = WrappedMPTConfig(d_model=256, n_heads=2, n_layers=2, expansion_ratio=4, max_seq_len=256, vocab_size=len(vocab), mm_hidden_size=96)
    torch.manual_seed(0)
    WrappedMPTForCausalLM(cfg).save_pretrained(str(ckpt))
    rng = np.random.default_rng(0)
    with tarfile.open(tmp_path / "s-000.tar", "w") as tf:
        for k in range(4):
            payload = json.dumps({"response": [{"question": "what is the genre ?", "answer": "it is jazz ." if k % 2 else "it is jazz rock piano ."}]}).encode()
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
            "--save_steps", "2", "--save_total_limit", "2", "--bf16", "True", "--report_to", "none", "--pack_sequences", "True"]
    with pytest.raises(NotImplementedError, match="--lora_enable"):
        T.main(argv + ["--lora_enable", "True"])
    T.main(argv)
    assert [os.path.basename(p) for p in CK.list_checkpoints(str(out))] == ["checkpoint-2", "checkpoint-3"]
    last = out / "checkpoint-3"
    sd = torch.load(last / "pytorch_model.bin")
    assert "transformer.blocks.1.attn.Wqkv.weight" in sd and "transformer.mm_projector.weight" in sd and not any(k.startswith("model.") for k in sd)
    assert (out / "mm_projector" / "checkpoint-3.bin").exists() and (last / "trainer_state.pt").exists() and (last / "config.json").exists()
    T.main([("4" if a == "3" else a) for a in argv])                     # --max_steps 4: resumes from checkpoint-3, one more step
    assert os.path.basename(CK.latest_checkpoint(str(out))) == "checkpoint-4"
    tok = AutoTokenizer.from_pretrained(str(last))
    model = WrappedMPTForCausalLM.from_pretrained(str(last), torch_dtype=torch.bfloat16)
    assert model.config.vocab_size == len(tok) == sd["transformer.wte.weight"].shape[0] and model.config.mm_hidden_size == 96
    now = model.state_dict()
    for k, v in sd.items():
        assert torch.equal(now[k].float(), v.bfloat16().float()), k
    base = WrappedMPTForCausalLM.from_pretrained(str(ckpt), torch_dtype=torch.bfloat16)
    assert not torch.equal(base.state_dict()["transformer.blocks.1.attn.Wqkv.weight"], now["transformer.blocks.1.attn.Wqkv.weight"])      # it trained
    model.cuda().eval()
    model.configure_engine(max_batch=1, max_seq=64)
    ids = torch.tensor([tok.convert_tokens_to_ids(["<s>", "what", "is", "the", "genre", "?"])])
    gen = model.generate(input_ids=ids.cuda(), max_new_tokens=5).cpu()
    assert gen.shape == (1, 11) and torch.equal(gen[:, :6], ids) and int(gen.max()) < len(tok)
