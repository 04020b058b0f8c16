"""The ragged slot mode of HipMptEngine (init_slots / prefill_slots / decode_slots / release_slots), the padded
WrappedMPTForCausalLM.generate and generate_inflight on an MPT model, against the CPU oracle (oracle.mpt_ref) run on every row ALONE --
never against the engine's own solo path.

Workload (built once on the CPU, ``_workload``): BASE of tests/test_mpt_gpu.py with audio tokens 93 / 94 / 95, the cases "alibi"
(make_weights seed 11) and "full" (qk_ln, clip_qkv 0.75, biases, alibi_bias_max 4, logit_scale 0.5; seed 21); eight rows of lengths
5, 9, 24, 37, 61, 16, 8, 33 drawn in that order from Generator(3) as randint(0, 90, (1, n)), rows with n >= 9 carrying a 4-frame audio
block (start token at column 1, four patch tokens, end token at column 6, randn(1, 4, 64) drawn right after the ids); 12 greedy tokens
per row.  The oracle's smallest top-2 logit margin over all 96 steps is 2.1e-3 (alibi) and 7.4e-3 (full) of max|logits| -- the
workload asserts >= 1e-3, ten times the split flow's bar of 1e-4 of max|ref| on each logit -- so the tokens must equal the oracle's on
EVERY step.
"""
import functools

import pytest
import torch

from conftest import report_close

pytestmark = pytest.mark.gpu

BASE = dict(d_model=256, n_heads=2, n_layers=2, expansion_ratio=4, vocab_size=96, max_seq_len=128, mm_hidden_size=64)
FULL = dict(qk_ln=True, clip_qkv=0.75, no_bias=False, alibi_bias_max=4, logit_scale=0.5)
LENS = [5, 9, 24, 37, 61, 16, 8, 33]
STEPS = 12
BUDGETS = [12, 3, 7, 12, 1, 9, 12, 5]


def _oracle_rows(MR, w, spec, rows, steps):
    """per row alone: logits [steps][V] (the prompt's last position, then one per fed token) and the greedy tokens [steps]"""
    out = []
    for ids, aud in rows:
        o = MR.forward(w, spec, ids, aud)
        lg, toks, past = [o["logits"][0, -1]], [], o["past_key_values"]
        for t in range(steps):
            toks.append(int(lg[-1].argmax()))
            if t + 1 < steps:
                o = MR.forward(w, spec, torch.tensor([[toks[-1]]]), None, past_key_values=past)
                past = o["past_key_values"]
                lg.append(o["logits"][0, -1])
        out.append((torch.stack(lg), toks))
    return out


@functools.lru_cache(maxsize=None)
def _workload(case):
    from oracle import mpt_ref as MR
    spec = MR.MptSpec(**BASE, audio_start_token=93, audio_end_token=94, audio_patch_token=95, **(FULL if case == "full" else {}))
    w = MR.make_weights(spec, seed=21 if case == "full" else 11)
    g = torch.Generator().manual_seed(3)
    rows = []
    for n in LENS:
        ids = torch.randint(0, 90, (1, n), generator=g)
        aud = None
        if n >= 9:
            ids[:, 1], ids[:, 2:6], ids[:, 6] = 93, 95, 94
            aud = torch.randn(1, 4, 64, generator=g)
        rows.append((ids, aud))
    ref = _oracle_rows(MR, w, spec, rows, STEPS)
    for r, (ids, aud) in enumerate(rows):
        assert ref[r][1] == MR.greedy_generate(w, spec, ids, aud, STEPS)[0, ids.shape[1]:].tolist()
    lg = torch.cat([lg for lg, _ in ref])
    top2 = lg.topk(2, dim=-1).values
    margin = float(((top2[:, 0] - top2[:, 1]) / lg.abs().amax(-1)).min())                 # of each step's own max|logits|, as the bar is
    assert margin >= 1e-3, f"{case}: top-2 margin {margin:.2e} of max|logits| is too close to the 1e-4 bar for token equality"
    return spec, w, rows, ref


def _engine(spec, w, precision="split", max_batch=8, max_seq=96):
    from llark_amd.m2t.mpt_engine import HipMptEngine, MptDims
    dims = MptDims(d_model=spec.d_model, n_heads=spec.n_heads, n_layers=spec.n_layers, expansion_ratio=spec.expansion_ratio,
                   vocab_size=spec.vocab_size, max_seq_len=spec.max_seq_len, alibi_bias_max=spec.alibi_bias_max, qk_ln=spec.qk_ln,
                   clip_qkv=spec.clip_qkv, logit_scale=spec.logit_scale, ln_eps=spec.ln_eps, mm_hidden_size=spec.mm_hidden_size)
    eng = HipMptEngine(dims, "cuda", max_batch, max_seq, precision=precision)
    eng.load_state_dict(w)
    return eng


def _segs(rows, which):
    return [(i, 1, rows[r][1][0].cuda()) for i, r in enumerate(which) if rows[r][1] is not None]


def _run_eight(eng, rows, steps=STEPS):
    """all rows at once, one slot each: [row] -> logits [steps][V] on the host"""
    n = len(rows)
    eng.init_slots(n)
    pre = eng.prefill_slots([ids[0].cuda() for ids, _ in rows], _segs(rows, range(n)), range(n))
    assert eng.slot_len_host == [ids.shape[1] for ids, _ in rows]
    got = [[pre[b].cpu()] for b in range(n)]
    nxt, _ = eng.advance_slots(pre, advance=False)
    for t in range(steps - 1):
        nxt, host, lg = eng.decode_slots(nxt)
        for b in range(n):
            got[b].append(lg[b].cpu())
    assert eng.slot_len_host == [ids.shape[1] + steps - 1 for ids, _ in rows]
    return [torch.stack(g) for g in got]


def _check_rows(name, got, ref):
    scale = max(float(lg.abs().max()) for lg, _ in ref)
    for r, (lg, toks) in enumerate(ref):
        for t in range(lg.shape[0]):
            report_close(f"{name} row {r} step {t}", got[r][t], lg[t], 1e-4 * float(lg[t].abs().max()))
        assert got[r].argmax(-1).tolist() == toks, f"{name} row {r}: tokens {got[r].argmax(-1).tolist()} vs oracle {toks}"


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", ["alibi", "full"])
def test_mpt_slots_match_the_oracle_row_by_row(case, fuse):
    """split flow, 8 slots: the prefill logits and every decode step's logits of every row within 1e-4 max|ref| of the oracle run on
    that row alone, tokens equal on every step; with the fused decode front and with the four-launch sequence"""
    spec, w, rows, ref = _workload(case)
    eng = _engine(spec, w)
    eng.fuse_decode_qk = fuse
    _check_rows(f"mpt slots {case} {'fused' if fuse else 'unfused'}", _run_eight(eng, rows), ref)


@pytest.mark.parametrize("case", ["alibi", "full"])
def test_mpt_slots_are_row_independent(case):
    """the same rows on 3 slots with release and refill, slots given out of order and as non-contiguous runs: per row bit-equal
    logits to the 8-slot run"""
    spec, w, rows, ref = _workload(case)
    eng = _engine(spec, w)
    eight = _run_eight(eng, rows)
    eng.init_slots(3)
    got = {r: [] for r in range(len(rows))}
    held, ids = {}, torch.zeros(3, dtype=torch.int64, device="cuda")

    def fill(which, slots):
        pre = eng.prefill_slots([rows[r][0][0].cuda() for r in which], _segs(rows, which), slots)
        for i, (r, b) in enumerate(zip(which, slots)):
            got[r].append(pre[i].cpu())
            held[b] = r
            ids[b] = pre[i].argmax()

    # slots 2 and 0: two runs of one row; later slot 1 alone; refills take whatever is free, highest slot first
    plan = [([0, 1], [2, 0]), ([2], [1])]
    queue = list(range(3, len(rows)))
    fill(*plan[0])
    step = 0
    while held:
        if step == 4:
            fill(*plan[1])
        nxt, host, lg = eng.decode_slots(ids)
        ids = nxt.clone()
        done = []
        for b, r in held.items():
            got[r].append(lg[b].cpu())
            if len(got[r]) == STEPS:
                done.append(b)
        if done:
            eng.release_slots(done)
            for b in done:
                del held[b]
        free = sorted((b for b in range(3) if b not in held), reverse=True)
        if queue and free and step >= 4:
            take = [queue.pop(0) for _ in range(min(len(free), len(queue)))]
            fill(take, free[:len(take)])
        step += 1
    for r in range(len(rows)):
        mine = torch.stack(got[r])
        assert torch.equal(mine, eight[r]), (f"{case} row {r}: max |diff| {float((mine - eight[r]).abs().max()):.3e} against the 8-slot run, "
                                             f"steps that differ: {[t for t in range(STEPS) if not torch.equal(mine[t], eight[r][t])]}")


def _wrapped(spec, w, max_batch, max_seq=96):
    from llark_amd.m2t.mpt import WrappedMPTConfig, WrappedMPTForCausalLM
    attn = dict(qk_ln=spec.qk_ln, clip_qkv=spec.clip_qkv, alibi_bias_max=spec.alibi_bias_max)
    cfg = WrappedMPTConfig(d_model=spec.d_model, n_heads=spec.n_heads, n_layers=spec.n_layers, expansion_ratio=spec.expansion_ratio,
                           max_seq_len=spec.max_seq_len, vocab_size=spec.vocab_size, mm_hidden_size=spec.mm_hidden_size, no_bias=spec.no_bias,
                           logit_scale=spec.logit_scale, attn_config=attn)
    m = WrappedMPTForCausalLM(cfg)
    m.load_state_dict(w, strict=True)
    ac = m.get_model().audio_encoder_config
    ac.use_audio_start_end, ac.audio_start_token, ac.audio_end_token, ac.audio_patch_token = True, 93, 94, 95
    m.cuda().eval()
    m.configure_engine(max_batch=max_batch, max_seq=max_seq)
    return m


@pytest.mark.parametrize("case", ["alibi", "full"])
def test_generate_inflight_on_an_mpt_model(case):
    """3 slots, budgets 12 .. 1: every yielded row is the prompt plus the oracle's tokens cut to its budget; slots are refilled"""
    from llark_amd.m2t.infer_driver import generate_inflight
    spec, w, rows, ref = _workload(case)
    m = _wrapped(spec, w, 3)
    examples = [(ids[0], None if aud is None else aud[0], BUDGETS[r]) for r, (ids, aud) in enumerate(rows)]
    trace = []
    got = dict(generate_inflight(m, iter(examples), slots=3, max_new_tokens=STEPS, keywords=(), trace=trace))
    assert sorted(got) == list(range(len(rows)))
    for r, (ids, _) in enumerate(rows):
        want = torch.cat((ids[0], torch.tensor(ref[r][1][:BUDGETS[r]], dtype=torch.int64)))
        assert torch.equal(got[r].cpu(), want), f"row {r}: {got[r].tolist()[ids.shape[1]:]} vs oracle {ref[r][1][:BUDGETS[r]]}"
    first_done = next(i for i, e in enumerate(trace) if e[0] == "done")
    assert any(e[0] == "prefill" for e in trace[first_done:]), "no slot was refilled"
    with pytest.raises(NotImplementedError, match="share_prefix"):
        list(generate_inflight(m, iter(examples), slots=3, max_new_tokens=2, keywords=(), share_prefix=True))


@pytest.mark.parametrize("left", [True, False], ids=["left_padded", "right_padded"])
def test_mpt_generate_with_a_padded_mask(left):
    """the first four rows as one padded batch: HF layout (the input as given, then the new tokens), tokens equal to the oracle's"""
    spec, w, rows, ref = _workload("full")
    m = _wrapped(spec, w, 4)
    four = rows[:4]
    S = max(ids.shape[1] for ids, _ in four)
    ids = torch.zeros((4, S), dtype=torch.int64)
    mask = torch.zeros((4, S), dtype=torch.int64)
    for b, (r, _) in enumerate(four):
        n = r.shape[1]
        sl = slice(S - n, S) if left else slice(0, n)
        ids[b, sl], mask[b, sl] = r[0], 1
    enc = [aud[0].cuda() for _, aud in four if aud is not None]
    got = m.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), audio_encodings=enc, max_new_tokens=STEPS).cpu()
    assert got.shape == (4, S + STEPS) and torch.equal(got[:, :S], ids)
    for b in range(4):
        assert got[b, S:].tolist() == ref[b][1], f"row {b}: {got[b, S:].tolist()} vs oracle {ref[b][1]}"
    assert m.engine.n_slots == 4
    # a row that emits EOS continues with the pad token
    eos = ref[1][1][2]
    stop = ref[1][1].index(eos)
    got = m.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), audio_encodings=enc, max_new_tokens=STEPS, eos_token_id=eos, pad_token_id=91).cpu()
    assert got[1, S:S + stop + 1].tolist() == ref[1][1][:stop + 1] and bool((got[1, S + stop + 1:] == 91).all())
    # prepare_inputs_for_generation keeps refusing right padding, forward any padded mask
    with pytest.raises(NotImplementedError, match="right padding"):
        m.prepare_inputs_for_generation(ids, attention_mask=torch.tensor([[1] * (S - 1) + [0]] * 4))
    with pytest.raises(NotImplementedError, match="padded batches"):
        m(input_ids=ids.cuda(), attention_mask=mask.cuda())


def test_mpt_generate_all_ones_mask_is_the_uniform_path():
    spec, w, rows, ref = _workload("full")
    m = _wrapped(spec, w, 4)
    ids, aud = rows[2]
    batch = ids.repeat(3, 1).cuda()
    enc = aud.repeat(3, 1, 1).cuda()
    a = m.generate(input_ids=batch, audio_encodings=enc, max_new_tokens=9)
    b = m.generate(input_ids=batch, attention_mask=torch.ones_like(batch), audio_encodings=enc, max_new_tokens=9)
    assert torch.equal(a, b) and a[0, ids.shape[1]:].tolist() == ref[2][1][:9]
    assert m.engine.n_slots == 0                                          # the slot mode was not entered


@functools.lru_cache(maxsize=1)
def _wide():
    """MPT-1B width (tests/test_mpt_gpu.py::test_mpt_1b_width_two_blocks) with qk_ln: 20 ragged rows of 3 .. 131 tokens, the oracle's
    prefill logits and two decode steps per row"""
    from oracle import mpt_ref as MR
    spec = MR.MptSpec(d_model=2048, n_heads=16, n_layers=2, expansion_ratio=4, vocab_size=512, max_seq_len=2048, mm_hidden_size=512,
                      qk_ln=True, audio_start_token=509, audio_end_token=510, audio_patch_token=511)
    w = MR.make_weights(spec, seed=1, std=0.02)
    g = torch.Generator().manual_seed(0)
    lens = [131, 3, 64, 17, 100, 8, 33, 128, 5, 71, 9, 40, 16, 127, 65, 12, 90, 7, 24, 3]
    rows = [(torch.randint(0, 500, (1, n), generator=g), None) for n in lens]
    return spec, w, rows, _oracle_rows(MR, w, spec, rows, 3)


@pytest.mark.parametrize("precision", ["split", "bf16"])
@pytest.mark.parametrize("n_slots", [20, 3])
def test_mpt_slots_at_1b_width(n_slots, precision):
    """20 slots run the decode products on gemm16_mid, 3 on gemm16: prefill and two decode steps against the oracle, 1e-4 max|ref| in
    the split flow, the bf16 flow's 3e-2 (tests/test_mpt_gpu.py::test_mpt_engine_bf16_flow_and_errors) otherwise"""
    spec, w, rows, ref = _wide()
    rows, ref = rows[:n_slots], ref[:n_slots]
    eng = _engine(spec, w, precision, max_batch=n_slots, max_seq=136)
    got = _run_eight(eng, rows, steps=3)
    assert (eng._slot_ws["mid"] is not None) == (n_slots > 16)
    for r, (lg, _) in enumerate(ref):
        for t in range(3):
            if precision == "split":
                report_close(f"1b width {n_slots} slots row {r} step {t}", got[r][t], lg[t], 1e-4 * float(lg[t].abs().max()))
            else:
                rel = float((got[r][t] - lg[t]).abs().max()) / float(lg[t].abs().max())
                assert rel < 3e-2, (r, t, rel)


def test_mpt_slot_mode_errors():
    from llark_amd.m2t.infer_driver import generate_inflight
    spec, w, rows, _ = _workload("alibi")
    eng = _engine(spec, w, max_batch=64, max_seq=16)
    with pytest.raises(ValueError, match="n_slots must be in 1 .. 64"):
        eng.init_slots(65)
    with pytest.raises(NotImplementedError, match="share_prefix"):
        eng.init_slots(2, share_prefix=True)
    with pytest.raises(RuntimeError, match="init_slots"):
        eng.decode_slots(torch.zeros(2, dtype=torch.int64, device="cuda"))
    eng.init_slots(2)
    pre = eng.prefill_slots([torch.arange(15).cuda()], (), [1])
    nxt = torch.stack((torch.zeros((), dtype=torch.int64, device="cuda"), pre[0].argmax()))
    nxt, _, _ = eng.decode_slots(nxt)                                      # position 15: the last one
    assert eng.slot_len_host == [-1, 16]
    with pytest.raises(ValueError, match=r"slot\(s\) \[1\] reached the engine's max_seq 16"):
        eng.decode_slots(nxt)
    with pytest.raises(ValueError, match="row lengths"):
        eng.prefill_slots([torch.arange(17).cuda()], (), [0])
    m = _wrapped(spec, w, 2)
    with pytest.raises(NotImplementedError, match="share_prefix"):
        list(generate_inflight(m, iter([(rows[0][0][0], None, 2)]), slots=2, keywords=(), share_prefix=True))
