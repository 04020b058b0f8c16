"""The ragged slot mode with more than 16 slots (17 .. 64: rmsnorm_bf16 + ops.gemm16_mid for every Linear of the decode step).
At Llama-2-7B widths 20 slots match each row's solo forward_tokens run at every step; a slot's logits are bit-identical whether 17 or
20 slots decode together; generate_inflight with 24 slots and slot refill returns per example what infer_with_prompt returns, and a
padded 20-row generate(attention_mask=...) what the solo runs return."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from toy_tokenizer import ToyTokenizer  # noqa: E402

pytestmark = pytest.mark.gpu

MM_CFG = dict(is_multimodal=True, sep_audio_conv_front=False, use_audio_start_end=True)
PROMPTS = ["Describe the tempo of this clip .", "What genre is it ?", "Name the instruments you hear in this recording and their roles .",
           "Is it loud ?"]
WORDS = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon".split()
MM = 96
SEED = 25                     # of the examples' encodings and budgets; the top-2 gap assertions below hold for it

# ---- Llama-2-7B widths, 2 layers ---------------------------------------------------------------------------------------------------
V = 1024
LENS = [5, 96, 17, 64, 33, 48, 9, 80, 25, 71, 12, 57, 40, 88, 21, 66, 7, 93, 30, 52]
FRAMES = {1: 40, 3: 20, 9: 30, 17: 60}                      # row -> audio frames
ORDER = [13, 2, 19, 7, 0, 16, 5, 11, 18, 3, 9, 14, 1, 6, 17, 10, 4, 15, 8, 12]      # slot k holds row ORDER[k]
STEPS = 4


@functools.lru_cache(maxsize=1)
def _weights_7b_width():
    from oracle import llama_ref as LR
    spec = LR.LlamaSpec(hidden_size=4096, intermediate_size=11008, num_hidden_layers=2, num_attention_heads=32,
                        vocab_size=V, mm_hidden_size=4800, audio_start_token=V - 2, audio_end_token=V - 1, audio_patch_token=V - 3)
    return spec, LR.make_weights(spec, seed=0, std=0.02, dtype=torch.bfloat16)


@functools.lru_cache(maxsize=2)
def _wide_run(precision):
    """Solo runs of the 20 rows (prefill + STEPS decode steps, greedy), then the same rows in 20 slots and the first 17 of them in 17
    slots, both fed the solo runs' tokens.  Computed once per precision and shared by the tests below."""
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    spec, w = _weights_7b_width()
    dims = LlamaDims(hidden_size=4096, intermediate_size=11008, num_hidden_layers=2, num_attention_heads=32, vocab_size=V,
                     rms_norm_eps=spec.rms_norm_eps, rope_theta=spec.rope_theta, mm_hidden_size=4800)
    eng = HipLlamaEngine(dims, "cuda", 20, 104, precision=precision)
    eng.load_state_dict(w)
    g = torch.Generator().manual_seed(7)
    rows, segs = [], {}
    for i, n in enumerate(LENS):
        F = FRAMES.get(i, 0)
        head = [1, V - 2] + [V - 3] * F + [V - 1] if F else [1]
        rows.append(torch.tensor(head + torch.randint(3, V - 3, (n - len(head),), generator=g).tolist()))
        assert rows[-1].numel() == n
        if F:
            segs[i] = (1, torch.randn(F, 4800, generator=g).cuda())
    solo, toks = [], []
    for i, r in enumerate(rows):
        sg = [(0,) + segs[i]] if i in segs else []
        lg = [eng.forward_tokens(r[None].cuda(), sg, last_only=True)[0, -1].cpu()]
        tk = [int(lg[-1].argmax())]
        for t in range(STEPS):
            lg.append(eng.forward_tokens(torch.tensor([[tk[-1]]]).cuda(), (), pos0=eng.cur_len, last_only=True)[0, -1].cpu())
            tk.append(int(lg[-1].argmax()))
        solo.append(torch.stack(lg))
        toks.append(tk)

    def slot_run(n_slots):
        """slot 0 is prefilled on its own (the same launches whatever n_slots is), slots 1 .. as one right-padded batch in shuffled order"""
        eng.init_slots(n_slots)
        order = ORDER[:n_slots]
        first = eng.prefill_slots([rows[order[0]].cuda()], [(0,) + segs[order[0]]] if order[0] in segs else [], slots=[0])
        rest = list(range(1, n_slots))
        shuffled = [rest[j] for j in torch.randperm(len(rest), generator=torch.Generator().manual_seed(3)).tolist()]
        pre = eng.prefill_slots([rows[order[k]].cuda() for k in shuffled],
                                [(j,) + segs[order[k]] for j, k in enumerate(shuffled) if order[k] in segs], slots=shuffled)
        assert eng.slot_len_host == [LENS[i] for i in order]
        got = [None] * n_slots
        got[0] = [first[0].cpu()]
        for j, k in enumerate(shuffled):
            got[k] = [pre[j].cpu()]
        for t in range(STEPS):
            ids = torch.tensor([toks[i][t] for i in order], dtype=torch.int64, device="cuda")       # the solo run's tokens: no row can diverge
            _, _, lg = eng.decode_slots(ids)
            lg = lg.cpu()
            for k in range(n_slots):
                got[k].append(lg[k].clone())
        assert eng.slot_len_host == [LENS[i] + STEPS for i in order]
        return [torch.stack(x) for x in got]

    return {"solo": solo, 20: slot_run(20), 17: slot_run(17)}


@pytest.mark.parametrize("precision", ["split", "bf16"])
def test_20_slots_at_7b_width_match_solo_forward(precision):
    """Every row, every step (the slot run is fed the solo run's tokens).  Bounds of
    tests/test_ragged_generate_gpu.py::test_slots_at_7b_width_match_solo_forward: 1e-4 of max|logits| (max and mean) in the "split"
    flow, max 1.5e-2 / mean 2e-3 in the "bf16" flow."""
    run = _wide_run(precision)
    worst = 0.0
    for k, i in enumerate(ORDER):
        ref, mine = run["solo"][i], run[20][k]
        scale = ref.abs().max().item()
        tol, tol_mean = (1e-4 * scale, 1e-4 * scale) if precision == "split" else (1.5e-2 * scale, 2e-3 * scale)
        for t in range(STEPS + 1):
            err, mean = (mine[t] - ref[t]).abs().max().item(), (mine[t] - ref[t]).abs().mean().item()
            worst = max(worst, err / tol, mean / tol_mean)
            assert err <= tol and mean <= tol_mean, f"slot {k} row {i} step {t}: |logits diff| max {err:.3e} mean {mean:.3e} (scale {scale:.3e})"
    print(f"[ratio] 20 slots vs solo, {precision}: worst error / bound = {worst:.3g}")
    for k in (17, 18, 19):                                                # a 16-row kernel silently reused would leave these rows unwritten
        for t in range(1, STEPS + 1):
            assert run[20][k][t].abs().max().item() > 0.0 and torch.isfinite(run[20][k][t]).all(), f"slot {k} step {t}: no logits"


@pytest.mark.parametrize("precision", ["split", "bf16"])
def test_a_slots_logits_do_not_depend_on_the_slot_count(precision):
    run = _wide_run(precision)
    a, b = run[20][0], run[17][0]
    assert a.shape == b.shape == (STEPS + 1, V)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "slot 0 differs between the 20-slot and the 17-slot run"


@pytest.mark.parametrize("precision", ["split", "bf16"])
def test_init_slots_range(precision):
    from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims
    dims = LlamaDims(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, vocab_size=128, mm_hidden_size=96)
    eng = HipLlamaEngine(dims, "cuda", 80, 32, precision=precision)
    with pytest.raises(ValueError, match="1 .. 64"):
        eng.init_slots(65)
    with pytest.raises(ValueError):
        eng.init_slots(0)
    eng = HipLlamaEngine(dims, "cuda", 24, 32, precision=precision)
    with pytest.raises(ValueError, match="1 .. 24"):
        eng.init_slots(25)
    eng.init_slots(24)
    assert eng.n_slots == 24


# ---- scheduler and wrapper, tiny model -----------------------------------------------------------------------------------------------
def _tok():
    from llark_amd.m2t.prompting import DEFAULT_CONVERSATION_HEADER
    tok = ToyTokenizer()
    for text in [DEFAULT_CONVERSATION_HEADER, "### Human: Assistant: <empty> \n " + " ".join(WORDS)] + PROMPTS:
        tok.encode(text)
    return tok


def _tiny_module(tok):
    """The host half of tests/test_ragged_generate_gpu.py::_tiny_model: weights scaled by 4 so that greedy choices are not near-ties."""
    from llark_amd.m2t.llamav2 import WrappedLlamav2Config, WrappedLlamav2ForCausalLM
    torch.manual_seed(0)
    cfg = WrappedLlamav2Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                               vocab_size=len(tok), max_position_embeddings=512, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.mm_hidden_size = MM
    m = WrappedLlamav2ForCausalLM(cfg).eval()
    m.get_model().initialize_adapter_modules()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((p * 4).bfloat16().float())
    m.initialize_audio_tokenizer(mm_use_audio_start_end=True, tokenizer=tok, device="cpu")
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.bfloat16().float())
    return m


def _tiny_model(tok, max_batch, max_seq):
    m = _tiny_module(tok)
    m.cuda()
    m.configure_engine(max_batch=max_batch, max_seq=max_seq)
    return m


def _examples(tok, end_seq, n=40, seed=SEED):
    from llark_amd.m2t.infer_driver import build_prompt_ids
    rng = np.random.default_rng(seed)
    examples, specs = [], []
    for i in range(n):
        text = PROMPTS[i % len(PROMPTS)]
        frames = [3, 40, 7, 90, 1, 25][i % 6]
        budget = int(rng.integers(1, 9))
        enc = torch.from_numpy(rng.standard_normal((frames, MM)).astype(np.float32))
        examples.append((build_prompt_ids(text, frames, tok, MM_CFG, end_seq, audio_first=True), enc, budget))
        specs.append((text, enc, budget))
    return examples, specs


class _GapRecorder:
    """A stopping criterion that never stops: records the solo run's top-2 logit gap over max|logits| at every generated step."""

    def __init__(self):
        self.worst = float("inf")

    def __call__(self, ids, scores):
        top2 = scores.float().topk(2, dim=-1).values
        self.worst = min(self.worst, float(((top2[:, 0] - top2[:, 1]) / scores.float().abs().amax(-1)).min()))
        return False


def _recording_generate(m, rec):
    orig = m.generate

    def generate(**kw):
        if kw.get("attention_mask") is None:                                      # solo runs only
            kw["stopping_criteria"] = [rec] + list(kw.get("stopping_criteria") or [])
        return orig(**kw)
    return generate


def test_generate_inflight_with_24_slots_equals_infer_with_prompt():
    from llark_amd.m2t.infer import infer_with_prompt
    from llark_amd.m2t.infer_driver import generate_inflight
    tok = _tok()
    end_seq = tok("\n### Assistant:").input_ids[1:]
    m = _tiny_model(tok, 24, 176)
    examples, specs = _examples(tok, end_seq)
    trace = []
    got = dict(generate_inflight(m, iter(examples), slots=24, tokenizer=tok, trace=trace))
    assert m.engine.n_slots == 24 and sorted(got) == list(range(40))
    prefills = [e for e in trace if e[0] == "prefill"]
    first_done = next(i for i, e in enumerate(trace) if e[0] == "done")
    assert len(prefills) > 1 and any(trace.index(p) > first_done for p in prefills), "no slot was refilled"
    rec = _GapRecorder()
    m.generate = _recording_generate(m, rec)
    for i, (text, enc, budget) in enumerate(specs):
        ref = infer_with_prompt(text, model=m, audio_encoding=enc, end_seq=end_seq, multimodal_cfg=MM_CFG, tokenizer=tok, audio_first=True,
                                max_new_tokens=budget).cpu()[0]
        assert torch.equal(got[i], ref), f"example {i}: ids differ: {got[i].tolist()} vs {ref.tolist()}"
    print(f"[ratio] solo runs: smallest top-2 gap / max|logits| = {rec.worst:.3g}")
    assert rec.worst >= 1e-3, "a solo greedy choice is a near-tie: change SEED, not the comparison"


def test_padded_generate_with_20_rows_equals_solo():
    tok = _tok()
    end_seq = tok("\n### Assistant:").input_ids[1:]
    m = _tiny_model(tok, 20, 176)
    examples, _ = _examples(tok, end_seq, n=20, seed=SEED + 1)
    rows, encs = [e[0] for e in examples], [e[1] for e in examples]
    N = 6
    rec = _GapRecorder()
    gen = _recording_generate(m, rec)
    solo = [gen(input_ids=r[None].cuda(), audio_encodings=e[None].cuda(), max_new_tokens=N).cpu()[0, r.numel():] for r, e in zip(rows, encs)]
    S = max(r.numel() for r in rows)
    ids = torch.zeros((20, S), dtype=torch.int64)
    mask = torch.zeros((20, S), dtype=torch.int64)
    for b, r in enumerate(rows):
        ids[b, S - r.numel():], mask[b, S - r.numel():] = r, 1                   # left-padded, the HF convention
    got = m.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), audio_encodings=[e.cuda() for e in encs], max_new_tokens=N).cpu()
    assert m.engine.n_slots == 20 and torch.equal(got[:, :S], ids)
    pad = m.generation_config.pad_token_id
    pad = m.generation_config.eos_token_id if pad is None else pad
    for b, s in enumerate(solo):
        assert torch.equal(got[b, S: S + s.numel()], s), f"row {b}: {got[b, S:].tolist()} vs solo {s.tolist()}"
        assert (got[b, S + s.numel():] == pad).all(), f"row {b}: a finished row must emit the pad token"
    print(f"[ratio] solo runs: smallest top-2 gap / max|logits| = {rec.worst:.3g}")
    assert rec.worst >= 1e-3, "a solo greedy choice is a near-tie: change SEED, not the comparison"
