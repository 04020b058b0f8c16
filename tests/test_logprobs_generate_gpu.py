"""GPU: token log-probabilities through the public surface -- the slot hook, ``generate_inflight(return_logprobs=True)``, both wrappers'
``generate(return_logprobs=True)``, ``score_continuations`` and ``shards --logprobs`` -- on the tiny models of
tests/test_sampling_generate_gpu.py.  Values are held to the float64 reference of tests/logprob_ref.py on the very logits the
kernel saw (cloned by a hook, or handed out through ``logits_sink``), within that module's tolerance."""
import io
import json
import tarfile

import numpy as np
import pytest
import torch

import logprob_ref as R
import test_mpt_slots_gpu as MG
import test_ragged_generate_gpu as LG
import test_sampling_generate_gpu as SG
import test_shared_prefix_gpu as SP

pytestmark = pytest.mark.gpu

N = SG.N


def _check_values(name, pairs, got):
    """pairs: [(fp32 logits row, token)]; got: the kernel's values for them."""
    assert len(pairs) == len(got), f"{name}: {len(got)} values for {len(pairs)} tokens"
    worst = 0.0
    for k, ((row, t), g) in enumerate(zip(pairs, got)):
        lp, _, _ = R.row_logprob(row, t)
        tol = R.tol_of(row, t)
        err = abs(float(g) - lp)
        worst = max(worst, err / tol)
        assert err <= tol, f"{name}: token {k} ({t}): {float(g)} vs {lp}, {err / tol:.3g} of tol"
    return worst


# ---- 1. the slot hook ------------------------------------------------------------------------------------------------------
def _drive(eng, prompts, segs_of, n_slots, budgets):
    """Greedy decoding of `prompts` on `n_slots` slots with refill, through decode_slots(sample=hook); the hook picks the token, calls the
    tracker and clones the step's logits.  Returns per example ([(logits row, token)], its history as take() gave it)."""
    from llark_amd import ops
    from llark_amd.m2t.logprob import LogprobTracker
    eng.init_slots(n_slots)
    vocab = eng.dims.vocab_size
    tracker = LogprobTracker(n_slots, vocab, eng.device, eng.smax)
    ids = torch.zeros((n_slots,), dtype=torch.int64, device="cuda")
    held, rec, hist = {}, {r: [] for r in range(len(prompts))}, {}
    queue = list(range(len(prompts)))
    cap, fills = [], []

    def fill(which, slots):
        pre = eng.prefill_slots([prompts[r].cuda() for r in which], segs_of(which), slots)
        first = pre.argmax(-1)
        tracker.admit(slots)
        tracker(pre, first, state=eng.slot_state, slot_of_row=slots)
        host, ft = pre.cpu().numpy(), first.cpu()
        for i, (r, b) in enumerate(zip(which, slots)):
            rec[r].append((host[i], int(ft[i])))
            held[b] = r
            ids[b] = first[i]
        fills.append(list(which))

    def hook(logits):
        toks = ops.sample_rows(logits, torch.zeros((n_slots,), dtype=torch.int64, device="cuda"), state=eng.slot_state, do_sample=False)
        tracker(logits, toks, state=eng.slot_state)
        cap.append((logits.clone(), toks.clone()))
        return toks

    def finish():
        done = [b for b, r in held.items() if len(rec[r]) == budgets[r]]
        if done:
            for b, h in zip(done, tracker.take(done)):
                hist[held.pop(b)] = h
            eng.release_slots(done)

    fill([queue.pop(0) for _ in range(n_slots)], list(range(n_slots)))
    finish()
    while held or queue:
        free = [b for b in range(n_slots) if b not in held]
        if queue and free:
            take = [queue.pop(0) for _ in range(min(len(free), len(queue)))]
            fill(take, free[:len(take)])
            finish()
            continue
        nxt, _, _ = eng.decode_slots(ids, sample=hook)
        ids = nxt.clone()
        lg, tk = cap.pop()
        lg, tk = lg.cpu().numpy(), tk.cpu()
        for b, r in held.items():
            assert int(tk[b]) == int(lg[b].argmax())
            rec[r].append((lg[b], int(tk[b])))
        finish()
    assert len(fills) >= 2, "no refill"
    return rec, hist


@pytest.mark.parametrize("n_slots", [1, 3, 17])
@pytest.mark.parametrize("backbone", ["llama", "mpt"])
def test_tracker_history_matches_the_reference_on_the_hooked_logits(backbone, n_slots):
    """17 slots take the mid-M decode GEMMs.  Budgets 1 .. 6: slots finish at different steps, and the examples beyond the slot count
    refill freed slots."""
    n = n_slots + 2
    budgets = [1 + (3 * r + 2) % 6 for r in range(n)]
    if backbone == "llama":
        tok = LG._tok()
        end_seq = tok("\n### Assistant:").input_ids[1:]
        m = LG._tiny_model(tok, max(n_slots, 2), 176)
        prompts = [LG._prompt(tok, end_seq, [5, 12, 30, 9, 21, 17, 44][r % 7], 0, None)[0] for r in range(n)]
        eng, segs_of = m.engine, (lambda which: [])
    elif n_slots > 16:                                         # MPT-1B width, the shapes tests/test_mpt_slots_gpu.py runs on gemm16_mid
        from oracle import mpt_ref as MR
        spec = MR.MptSpec(d_model=2048, n_heads=16, n_layers=2, expansion_ratio=4, vocab_size=512, max_seq_len=2048, mm_hidden_size=512,
                          qk_ln=True, audio_start_token=509, audio_end_token=510, audio_patch_token=511)
        w = MR.make_weights(spec, seed=1, std=0.02)
        g = torch.Generator().manual_seed(0)
        rows = [(torch.randint(0, 500, (1, k), generator=g), None) for k in (31, 3, 64, 17, 40, 8, 33)]
        eng = MG._engine(spec, w, max_batch=n_slots, max_seq=72)
        pick = [r % len(rows) for r in range(n)]
        prompts = [rows[r][0][0] for r in pick]
        segs_of = lambda which: []                                                # noqa: E731
    else:
        spec, w, rows, _ = MG._workload("full")
        eng = MG._engine(spec, w, max_batch=max(n_slots, 2))
        pick = [r % len(rows) for r in range(n)]
        prompts = [rows[r][0][0] for r in pick]
        segs_of = lambda which: MG._segs(rows, [pick[r] for r in which])          # noqa: E731
    rec, hist = _drive(eng, prompts, segs_of, n_slots, budgets)
    worst = 0.0
    for r in range(n):
        assert hist[r].numel() == budgets[r] == len(rec[r]) and hist[r].dtype == torch.float32
        worst = max(worst, _check_values(f"{backbone} {n_slots} slots example {r}", rec[r], hist[r].tolist()))
    print(f"[ratio] tracker {backbone} {n_slots} slots: worst logprob error {worst:.3g} of tol")


# ---- 2-4. generate_inflight ------------------------------------------------------------------------------------------------
def _llama_examples(tok, end_seq, n=5, seed=21):
    from llark_amd.m2t.infer_driver import build_prompt_ids
    rng = np.random.default_rng(seed)
    examples = []
    for i in range(n):
        frames = [3, 40, 7, 90, 1, 25][i % 6]
        enc = torch.from_numpy(rng.standard_normal((frames, LG.MM)).astype(np.float32))
        examples.append((build_prompt_ids(LG.PROMPTS[i % 4], frames, tok, LG.MM_CFG, end_seq, audio_first=True), enc, [4, 9, 2, 7, 5][i % 5]))
    return examples


def _mpt_examples(rows, n=5):
    return [(ids[0], None if aud is None else aud[0], MG.BUDGETS[r]) for r, (ids, aud) in enumerate(rows[:n])]


def _inflight_pair(m, examples, slots, **kw):
    from llark_amd.m2t.infer_driver import generate_inflight
    plain = dict(generate_inflight(m, iter(examples), slots=slots, max_new_tokens=MG.STEPS, **kw))
    with_lp = {i: (ids, lp) for i, ids, lp in generate_inflight(m, iter(examples), slots=slots, max_new_tokens=MG.STEPS, return_logprobs=True, **kw)}
    assert sorted(plain) == sorted(with_lp) == list(range(len(examples)))
    for i, ex in enumerate(examples):
        ids, lp = with_lp[i]
        assert torch.equal(ids, plain[i]), f"example {i}: tokens changed with return_logprobs"
        assert lp.dtype == torch.float32 and lp.dim() == 1 and lp.numel() == ids.numel() - ex[0].numel() >= 1
        assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()), (i, lp)
    return with_lp


@pytest.mark.parametrize("backbone", ["llama", "mpt"])
def test_generate_inflight_returns_logprobs_and_keeps_the_tokens(backbone):
    from llark_amd.m2t.sampling import SamplingParams
    if backbone == "llama":
        tok, end_seq, m, _, _ = SG._llama()
        examples, kw = _llama_examples(tok, end_seq), dict(tokenizer=tok)
    else:
        m, rows, _ = SG._mpt(3)
        examples, kw = _mpt_examples(rows), dict(keywords=())
    greedy = _inflight_pair(m, examples, 3, **kw)
    sp = SamplingParams(do_sample=True, temperature=1.2, top_k=40, top_p=0.95, repetition_penalty=1.1, seed=4)
    drawn = _inflight_pair(m, examples, 3, sampling=sp, **kw)
    assert any(not torch.equal(greedy[i][0], drawn[i][0]) for i in greedy)
    if backbone == "mpt":                                      # budgets are the only stop: every length is its budget
        assert [greedy[i][1].numel() for i in range(5)] == MG.BUDGETS[:5]


def test_mpt_logprobs_do_not_depend_on_the_slot_count():
    """MPT's prefill and decode logits are bit-equal whatever slot a row rides in (test_mpt_slots_are_row_independent), and the kernel's
    value depends on the row's floats and the token alone: 1 slot and 3 slots give bit-equal log-probabilities."""
    from llark_amd.m2t.infer_driver import generate_inflight
    m, rows, _ = SG._mpt(3)
    examples = _mpt_examples(rows, 8)
    run = lambda n: {i: (ids, lp) for i, ids, lp in generate_inflight(m, iter(examples), slots=n, max_new_tokens=MG.STEPS, keywords=(),      # noqa: E731
                                                                     return_logprobs=True)}
    one, three = run(1), run(3)
    for i in range(len(examples)):
        assert torch.equal(one[i][0], three[i][0])
        assert torch.equal(one[i][1].view(torch.int32), three[i][1].view(torch.int32)), f"example {i}: {one[i][1]} vs {three[i][1]}"


def test_llama_forked_siblings_get_their_first_token_entry():
    from llark_amd.m2t.infer_driver import generate_inflight
    tok = SP._tok()
    end_seq = tok("\n### Assistant:").input_ids[1:]
    m = SP._tiny_model(tok, 4, 256)
    examples = SP._clip_examples(tok, end_seq, n=8)            # clip 0 (audio first): its questions fork; clip 1: full prefills
    trace = []
    got = {i: (ids, lp) for i, ids, lp in generate_inflight(m, iter(examples), slots=4, tokenizer=tok, trace=trace, share_prefix=True,
                                                           return_logprobs=True)}
    plain = dict(generate_inflight(m, iter(examples), slots=4, tokenizer=tok, share_prefix=True))
    forks = [e for e in trace if e[0] == "fork"]
    assert forks, "nothing was forked"
    forked_idx = set()
    for e in forks:
        nxt = next(p for p in trace[trace.index(e):] if p[0] == "prefill")
        forked_idx.add(nxt[2][nxt[1].index(e[2])])
    for i, ex in enumerate(examples):
        ids, lp = got[i]
        assert torch.equal(ids, plain[i])
        assert lp.numel() == ids.numel() - ex[0].numel() >= 1 and bool(torch.isfinite(lp).all()), (i, i in forked_idx, lp)


# ---- 5. generate -----------------------------------------------------------------------------------------------------------
def _check_generate(name, m, kw, S, eos, may_pad=True, **extra):
    torch.manual_seed(5)
    plain = m.generate(**kw, eos_token_id=eos, **extra)
    torch.manual_seed(5)
    ids, lp = m.generate(**kw, eos_token_id=eos, return_logprobs=True, **extra)
    assert torch.equal(ids, plain), f"{name}: tokens changed with return_logprobs"
    new = ids[:, S:].cpu()
    assert lp.is_cuda and lp.dtype == torch.float32 and tuple(lp.shape) == tuple(new.shape)
    lp = lp.cpu()
    want_nan = torch.zeros(new.shape, dtype=torch.bool)
    for b in range(new.shape[0]):
        hit = (new[b] == eos).nonzero()
        if may_pad and hit.numel():
            want_nan[b, int(hit[0]) + 1:] = True                # after its EOS a row emits padding
    assert torch.equal(torch.isnan(lp), want_nan), f"{name}: NaN at {torch.isnan(lp).nonzero().tolist()}, padding at {want_nan.nonzero().tolist()}"
    assert bool((lp[~want_nan] <= 0).all()) and bool(torch.isfinite(lp[~want_nan]).all())
    return new, want_nan


def test_llama_generate_returns_logprobs():
    tok, end_seq, m, rows, encs = SG._llama()
    for name, kw in (("uniform", SG._llama_uniform(m, tok, end_seq)), ("left-padded", SG._llama_padded(rows, encs))):
        S = kw["input_ids"].shape[1]
        free = m.generate(**kw, eos_token_id=-1)[:, S:].cpu()
        eos = int(free[0, 2])                                     # row 0 stops after its third token, then emits padding
        new, nan = _check_generate(f"llama {name} greedy", m, kw, S, eos)
        assert bool(nan.any()) and not bool(nan.all()), f"llama {name}: the case emits no padding"
        _check_generate(f"llama {name} device sampler", m, kw, S, eos, do_sample=True, temperature=1.3, top_p=0.9, seed=3)
        _check_generate(f"llama {name} multinomial", m, kw, S, eos, do_sample=True, temperature=1.3)


def test_mpt_generate_returns_logprobs():
    m, rows, _ = SG._mpt()
    kw = SG._mpt_uniform(rows)
    S = kw["input_ids"].shape[1]
    free = m.generate(**kw)[:, S:].cpu()
    _check_generate("mpt uniform greedy", m, kw, S, int(free[0, -1]) + 1000, may_pad=False)      # the uniform MPT loop emits no padding
    _check_generate("mpt uniform sampler", m, kw, S, -1, may_pad=False, do_sample=True, top_p=0.9, seed=1)
    kw = SG._mpt_padded(rows)
    S = kw["input_ids"].shape[1]
    free = m.generate(**kw)[:, S:].cpu()
    eos = int(free[1, 3])
    new, nan = _check_generate("mpt left-padded greedy", m, kw, S, eos)
    assert bool(nan.any()) and not bool(nan.all())
    _check_generate("mpt left-padded sampler", m, kw, S, eos, do_sample=True, top_p=0.9, seed=1)


# ---- 6. score_continuations ------------------------------------------------------------------------------------------------
LENGTHS = [3, 1, 6, 4, 3]                                          # four different lengths, and one that repeats (MPT batches the pair)


def _check_scores(name, model, prompt, enc, conts, max_batch):
    from llark_amd.m2t.infer_driver import score_continuations
    sink = []
    got = score_continuations(model, prompt, enc, conts, logits_sink=sink)
    P = prompt.numel()
    assert len(got) == len(conts) and all(g.dtype == torch.float32 and not g.is_cuda and g.numel() == len(c) for g, c in zip(got, conts))
    # spans: every call's tokens are -1 except, per candidate row, its own ids from the prompt's last position on
    scored = {}
    seen_rows = 0
    for logits, tokens in sink:
        assert logits.dim() == 2 and tokens.shape == (logits.shape[0],) and len(sink) >= 2
        tk = tokens.cpu()
        lg = logits.cpu().numpy()
        rows = (tk >= 0).nonzero().view(-1).tolist()
        runs = []
        for r in rows:
            if runs and r == runs[-1][-1] + 1:
                runs[-1].append(r)
            else:
                runs.append([r])
        S = P + max(len(run) for run in runs)                    # the call's sequence length: the prompt and its longest candidate
        assert logits.shape[0] % S == 0 and logits.shape[0] // S == len(runs) <= max_batch, f"{name}: {logits.shape[0]} rows, S = {S}, {len(runs)} spans"
        for run in runs:
            want = tk[run].tolist()
            match = [i for i, c in enumerate(conts) if list(c) == want and i not in scored]
            assert match, f"{name}: scored span {want} is no candidate"
            i = match[0]
            assert run[0] % S == P - 1, f"{name}: candidate {i} starts at row {run[0] % S}, the prompt's last position is {P - 1}"
            scored[i] = [(lg[r], int(tk[r])) for r in run]
        seen_rows += len(rows)
    assert sorted(scored) == list(range(len(conts))) and seen_rows == sum(len(c) for c in conts), "pad or prompt rows were scored"
    worst, sums, tols = 0.0, [], []
    for i in range(len(conts)):
        worst = max(worst, _check_values(f"{name} candidate {i}", scored[i], got[i].tolist()))
        sums.append(sum(R.row_logprob(row, t)[0] for row, t in scored[i]))
        tols.append(sum(R.tol_of(row, t) for row, t in scored[i]))
    print(f"[ratio] score_continuations {name}: worst logprob error {worst:.3g} of tol")
    order = np.argsort(sums)[::-1]
    if sums[order[0]] - sums[order[1]] > tols[order[0]] + tols[order[1]]:
        assert int(np.argmax([float(g.double().sum()) for g in got])) == int(order[0])
    return got


def test_score_continuations_llama():
    from llark_amd.m2t.infer_driver import build_prompt_ids
    tok, end_seq, m, _, _ = SG._llama()
    words = [tok.vocab[w] for w in LG.WORDS]
    enc = torch.from_numpy(np.random.default_rng(2).standard_normal((7, LG.MM)).astype(np.float32))
    prompt = build_prompt_ids(LG.PROMPTS[1], 7, tok, LG.MM_CFG, end_seq, audio_first=True)
    conts = [[words[(5 * i + k) % len(words)] for k in range(n)] for i, n in enumerate(LENGTHS)]
    got = _check_scores("llama", m, prompt, enc, conts, 4)
    # in another order (other batch mates, another padded length) a candidate scores the same tokens to within the engine's own noise
    again = _check_scores("llama, reordered", m, prompt, enc, [conts[2], conts[4], conts[0], conts[3], conts[1]], 4)
    assert abs(float(again[0].sum()) - float(got[2].sum())) <= 1e-3 * abs(float(got[2].sum()))


def test_score_continuations_mpt():
    m, rows, _ = SG._mpt()
    ids, aud = rows[2]
    conts = [[(7 * i + 3 * k + 1) % 90 for k in range(n)] for i, n in enumerate(LENGTHS)]
    _check_scores("mpt", m, ids[0], aud[0], conts, 4)


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------------
def test_shards_cli_logprobs(tmp_path):
    """`shards --logprobs` on a two-example shard adds the three columns, finite; without the flag the CSV has today's columns and the
    same texts."""
    import pandas as pd
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from llark_amd.m2t import infer_driver as D
    from llark_amd.m2t.llamav2 import WrappedLlamav2Config, WrappedLlamav2ForCausalLM
    from llark_amd.m2t.prompting import DEFAULT_CONVERSATION_HEADER
    words = sorted(set((DEFAULT_CONVERSATION_HEADER + " ### Human: Assistant: <empty> what is k0 ? it . tempo fast").split()))
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "\n": 3}
    for wd in words:
        vocab.setdefault(wd, len(vocab))
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    ckpt = tmp_path / "ckpt"
    PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", bos_token="<s>", eos_token="</s>").save_pretrained(str(ckpt))
    cfg = WrappedLlamav2Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                               vocab_size=len(vocab), max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.mm_hidden_size = 96
    torch.manual_seed(0)
    WrappedLlamav2ForCausalLM(cfg).save_pretrained(str(ckpt))
    buf = io.BytesIO()
    np.save(buf, np.random.default_rng(3).standard_normal((4, 96)).astype(np.float32))
    with tarfile.open(tmp_path / "s-000.tar", "w") as tf:
        resp = {"response": [{"question": "what is k0 ?", "answer": "it is k0 ."}, {"question": "tempo ?", "answer": "fast ."}]}
        SG._add(tf, "k0.json", json.dumps(resp).encode())
        SG._add(tf, "k0.audio_encoding.npy", buf.getvalue())
    out, out_lp = tmp_path / "res" / "out.csv", tmp_path / "res" / "out_lp.csv"
    args = ["--model_name_or_path", str(ckpt), "--eval_data_path", str(tmp_path / "s-000.tar"), "--max_new_tokens", "6", "--slots", "2",
            "--mm_hidden_size", "96", "--model_max_length", "128"]
    torch.manual_seed(1)                        # loading draws the embedding rows of the added tokens from torch's generator
    recs = D.main_shards(args + ["--outfile", str(out)])
    torch.manual_seed(1)
    recs_lp = D.main_shards(args + ["--outfile", str(out_lp), "--logprobs"])
    df, df_lp = pd.read_csv(out, keep_default_na=False), pd.read_csv(out_lp, keep_default_na=False)
    assert list(df.columns) == D.SHARD_COLUMNS and all(set(r) == set(D.SHARD_COLUMNS) for r in recs)
    assert list(df_lp.columns) == D.SHARD_COLUMNS + ["sum_logprob", "mean_logprob", "n_tokens"] and len(df_lp) == 2
    assert df_lp[D.SHARD_COLUMNS].equals(df)
    for r in recs_lp:
        assert 1 <= r["n_tokens"] <= 6 and np.isfinite(r["sum_logprob"]) and r["sum_logprob"] <= 0
        assert abs(r["mean_logprob"] - r["sum_logprob"] / r["n_tokens"]) <= 1e-9 * abs(r["sum_logprob"])
    assert np.isfinite(df_lp[["sum_logprob", "mean_logprob"]].to_numpy(dtype=np.float64)).all()
