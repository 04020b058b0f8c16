"""GPU: guided choice through the public surface -- both wrappers' ``generate(allowed_continuations=...)`` (uniform, padded, sampled,
beams on Llama) and ``generate_inflight(choice_sets=...)`` -- on the tiny models of tests/test_constrain_generate_gpu.py.

The host loop: a stopping criterion that never stops receives, after every token, the ids so far and the RAW logits the token was chosen
from.  tests/guide_ref.py walked along each row's own tokens and applied to those logits, then argmax, must give the token ``generate``
chose; every completion must be a member of its row's set followed by the EOS."""
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import guide_ref as GR
import test_constrain_generate_gpu as CG
import test_ragged_generate_gpu as LG

pytestmark = pytest.mark.gpu

EOS, N = 2, 6
BEAM_TOL = 7.93e-5                                                 # test_guided_beams_find_the_best_member: twice the measured 3.964e-05
SET_A = [[10, 11, 12], [10, 11], [10, 13], [14], [15, 16, 17]]     # [10, 11] is whole and a prefix of [10, 11, 12]
SET_B = [[20, 21], [22], [20, EOS, 23]]                            # eos as a non-final member: the EOS rule ends the row there
MEMBERS_B = [[20, 21], [22], [20]]                                 # ... so what a row of SET_B can show before its EOS


def _kw(name):
    m, kw, rows = CG._cases()[name]
    kw = {k: v for k, v in kw.items() if k != "eos_token_id"}
    if name.startswith("mpt"):
        kw["pad_token_id"] = 0
    return m, dict(kw, max_new_tokens=N, eos_token_id=EOS), rows


def _completion(tokens):
    """The row's new tokens up to its first EOS (without it), and whether there was one."""
    tokens = [int(t) for t in tokens]
    return (tokens[:tokens.index(EOS)], True) if EOS in tokens else (tokens, False)


def _check_members(out, S, sets, members=None):
    for b, s in enumerate(sets):
        if s is None:
            continue
        got, ended = _completion(out[b, S:].tolist())
        ok = members[b] if members is not None else s
        assert ended and got in [list(q) for q in ok], f"row {b}: {out[b, S:].tolist()} is no member of {ok} followed by the EOS"


def _check_host_loop(tap, sets, S, argmax=True, ngram=0, rows=None):
    """Every token of a guided row is the first maximum of its step's raw logits with -inf outside what the restatement allows after the
    row's own tokens (argmax False: it only is an allowed one).  ``ngram``: composed with constrain_ref's bigram ban, applied first."""
    assert len(tap.steps) >= 2
    for b, s in enumerate(sets):
        g = GR.RowGuide(s, EOS)
        for t, (ids, scores) in enumerate(tap.steps):
            tokn = int(ids[b, S + t])
            row = scores[b].numpy()
            if ngram:
                hist = rows[b].tolist() + ids[b, S:S + t].tolist()
                row = CR.processed_row(row, CR.banned_set(hist, len(row), n=ngram))
            assert g.allowed(len(row))[tokn], f"row {b} step {t}: token {tokn} is not allowed after {ids[b, S:S + t].tolist()}"
            if argmax:
                want = int(np.argmax(g.mask(row)))
                assert tokn == want, f"row {b} step {t}: {tokn} vs the host loop's {want}"
            g.push(tokn)
            if tokn == EOS:
                break
        assert g.status == 0


@pytest.mark.parametrize("name", CG.CASES)
def test_greedy_completions_are_members_and_equal_a_host_loop(name):
    m, kw, rows = _kw(name)
    S = kw["input_ids"].shape[1]
    plain = m.generate(**kw)
    assert torch.equal(m.generate(**kw, allowed_continuations=None), plain)          # absent: the bits of the plain run
    tap = CG._Tap()
    got = m.generate(**kw, stopping_criteria=[tap], allowed_continuations=[SET_A, SET_B])      # one set per row
    _check_members(got, S, [SET_A, SET_B], [SET_A, MEMBERS_B])
    _check_host_loop(tap, [SET_A, SET_B], S)
    one = m.generate(**kw, allowed_continuations=SET_A)                               # one set for every row
    _check_members(one, S, [SET_A, SET_A])
    assert one[0, S:S + 2].tolist() == got[0, S:S + 2].tolist()
    # a None row is unconstrained: its tokens are the plain run's, the other row's are its guided ones
    tap = CG._Tap()
    mixed = m.generate(**kw, stopping_criteria=[tap], allowed_continuations=[SET_A, None])
    _check_members(mixed, S, [SET_A, None])
    w = min(mixed.shape[1], plain.shape[1])
    free, _ = _completion(plain[1, S:w].tolist())
    assert mixed[1, S:S + len(free)].tolist() == free, f"the unconstrained row changed: {mixed[1, S:].tolist()} vs {plain[1, S:].tolist()}"
    _check_host_loop(tap, [SET_A, None], S)


@pytest.mark.parametrize("name", CG.CASES)
def test_seeded_sampled_completions_are_members_and_repeat(name):
    m, kw, rows = _kw(name)
    S = kw["input_ids"].shape[1]
    more = dict(do_sample=True, temperature=1.5, top_k=8, top_p=0.95, seed=11, allowed_continuations=[SET_A, SET_B])
    tap = CG._Tap()
    a = m.generate(**kw, stopping_criteria=[tap], **more)
    b = m.generate(**kw, **more)
    assert torch.equal(a, b), "the same seed gave two outputs"
    _check_members(a, S, [SET_A, SET_B], [SET_A, MEMBERS_B])
    _check_host_loop(tap, [SET_A, SET_B], S, argmax=False)
    seen = {tuple(_completion(m.generate(**kw, **dict(more, seed=s))[0, S:].tolist())[0]) for s in range(6)}
    assert len(seen) > 1, "six seeds drew one and the same member"


def test_llama_multinomial_path_reads_the_guided_row():
    m, kw, rows = _kw("llama_uniform")
    S = kw["input_ids"].shape[1]
    torch.manual_seed(3)
    tap = CG._Tap()
    got = m.generate(**kw, stopping_criteria=[tap], do_sample=True, temperature=2.0, allowed_continuations=[SET_A, SET_B])
    _check_members(got, S, [SET_A, SET_B], [SET_A, MEMBERS_B])
    _check_host_loop(tap, [SET_A, SET_B], S, argmax=False)


@pytest.mark.parametrize("name", CG.CASES)
def test_composition_with_no_repeat_ngram_size(name):
    """The bigram ban comes first, the guide second: a set whose members repeat a bigram of the row's own tokens loses them."""
    m, kw, rows = _kw(name)
    S = kw["input_ids"].shape[1]
    kw["max_new_tokens"] = 7
    used = {int(t) for r in rows for t in r.tolist()} | {EOS}
    a, b, c, d, e, f, g = [t for t in range(3, 60) if t not in used][:7]              # tokens no prompt holds: no bigram of theirs is banned yet
    sets = [[[a, b, a, b, c], [a, b, a, d]], [[e, e, f], [e, g]]]                    # row 0: (a, b) twice is banned; row 1: free of repeats
    tap = CG._Tap()
    got = m.generate(**kw, stopping_criteria=[tap], no_repeat_ngram_size=2, allowed_continuations=sets)
    _check_host_loop(tap, sets, S, ngram=2, rows=rows)
    assert _completion(got[0, S:].tolist()) == ([a, b, a, d], True)
    _check_members(got, S, sets)
    # every continuation banned: the row has no finite logit left, and the call says so instead of emitting a token
    with pytest.raises(RuntimeError, match="no allowed token left"):
        m.generate(**kw, no_repeat_ngram_size=2, allowed_continuations=[[[a, a, a, a]], [[g]]])


@pytest.mark.parametrize("name", ["llama_uniform", "mpt_padded"])
def test_absent_argument_builds_nothing(name, monkeypatch):
    from llark_amd.m2t import choice as C
    m, kw, rows = _kw(name)
    plain = m.generate(**kw)

    def boom(*a, **k):
        raise AssertionError("a guide was built")
    monkeypatch.setattr(C, "DeviceGuide", boom)
    assert torch.equal(m.generate(**kw, allowed_continuations=None), plain)
    assert C.TokenChooser.build(2, 64, "cuda", sampling=None, constraints=None, guide=None, logprobs=False, choose=lambda r: r.argmax(-1)) is None
    with pytest.raises(ValueError, match="a choice set needs eos_token_id >= 0"):
        m.generate(**dict(kw, eos_token_id=-1), allowed_continuations=SET_A)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="outside \\[0, vocab"):
        m.generate(**kw, allowed_continuations=[[10 ** 6]])
    if name.startswith("mpt"):
        with pytest.raises(NotImplementedError, match="beam search is not implemented for MPT"):
            m.generate(**kw, num_beams=2, allowed_continuations=SET_A)


def _with_eos(m):
    gc = getattr(m, "generation_config", None)
    if gc is None:
        m.generation_config = types.SimpleNamespace(eos_token_id=EOS)
        return lambda: setattr(m, "generation_config", None)
    old = gc.eos_token_id
    gc.eos_token_id = EOS
    return lambda: setattr(gc, "eos_token_id", old)


@pytest.mark.parametrize("kind", ["llama", "mpt"])
def test_inflight_completions_are_members_and_do_not_depend_on_the_slot_count(kind):
    from llark_amd.m2t.infer_driver import generate_inflight
    m, tok, ex = CG._inflight_examples(kind)
    which = [0, None, 1, 0, 1, None, 0, 1, 0, None, 1, 0]
    ex = [(e[0], e[1], max(e[2], 5), e[3] if len(e) > 3 else None, which[i]) for i, e in enumerate(ex)]
    sets = [SET_A, SET_B]
    restore = _with_eos(m)
    try:
        def run(n, **kw):
            return dict(generate_inflight(m, iter(ex), slots=n, max_new_tokens=N, keywords=(), choice_sets=sets, **kw))
        one, three = run(1), run(3)
        plain = dict(generate_inflight(m, iter([e[:4] for e in ex]), slots=3, max_new_tokens=N, keywords=()))
        lp = {o[0]: o for o in generate_inflight(m, iter(ex), slots=3, max_new_tokens=N, keywords=(), choice_sets=sets, return_logprobs=True)}
    finally:
        restore()
    assert sorted(one) == sorted(three) == list(range(len(ex)))
    for i, e in enumerate(ex):
        assert torch.equal(one[i], three[i]), f"example {i}: {one[i].tolist()} with 1 slot, {three[i].tolist()} with 3"
        new = three[i][e[0].numel():].tolist()
        if e[4] is None:                                           # unconstrained: the plain run's tokens
            assert torch.equal(three[i], plain[i]), f"example {i}: an unconstrained example changed"
        else:
            assert new[-1] == EOS and new[:-1] in [SET_A, MEMBERS_B][e[4]], f"example {i}: {new} is no member of set {e[4]} followed by the EOS"
        assert torch.equal(lp[i][1], three[i]) and lp[i][2].numel() == len(new) and bool(torch.isfinite(lp[i][2]).all())
    assert any(e[4] is not None and not torch.equal(plain[i], three[i]) for i, e in enumerate(ex))


def test_guided_beams_find_the_best_member():
    """Llama, ``num_beams`` >= the set's size, ``length_penalty=0``: the returned hypothesis is a member followed by the EOS, and its summed
    log-probability (the member's tokens and the closing EOS, which is what the search maximises) reaches the maximum that
    ``score_continuations(member + [EOS]).sum()`` finds over the set.  Scores are compared, not identities: near-ties need no skipping.

    Tolerance: tests/test_logprobs_generate_gpu.py holds both paths to a float64 reference but sets no bound between them, so it was
    measured: on these two prompts, unguided ``generate(num_beams=4, length_penalty=0, return_logprobs=True)`` against ``score_continuations`` of the very
    tokens it returned (2, 4 and 6 new tokens, with and without the EOS; greedy and 2 beams gave the same figures) differ by at most
    3.964e-05 in the sum and 3.189e-05 in one token (the decode steps read the K/V cache the prefill wrote, the scorer runs one
    prefill over prompt and candidate); twice the sum's figure is allowed: 7.93e-05."""
    from llark_amd.m2t.infer_driver import score_continuations
    tok, m = CG._llama()
    rows = CG._llama_rows()
    ids, mask = LG._padded(rows, True)
    S = ids.shape[1]
    sets = [[[10, 11, 12], [10, 11], [10, 13], [14]], [[20, 21], [22], [23, 24, 25], [23, 24]]]
    B = 4                                                          # as many beams as members; 2 x 4 slots, the tiny engine's 8
    out, lps = m.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), max_new_tokens=N, num_beams=B, length_penalty=0.0,
                          return_logprobs=True, eos_token_id=EOS, allowed_continuations=sets)
    _check_members(out, S, sets)
    worst = []
    for b, s in enumerate(sets):
        got = float(torch.nan_to_num(lps[b].double().cpu(), nan=0.0).sum())
        member, _ = _completion(out[b, S:].tolist())
        assert int(torch.isfinite(lps[b]).sum()) == len(member) + 1
        sums = [float(x.double().sum()) for x in score_continuations(m, rows[b], None, [list(q) + [EOS] for q in s])]
        print(f"[guided beams] example {b}: returned {member} sum {got:.6f}; scorer's best {max(sums):.6f} "
              f"({s[int(np.argmax(sums))]}), all {[round(x, 4) for x in sums]}")
        worst.append(abs(got - max(sums)))
    assert max(worst) <= BEAM_TOL, f"|returned sum - the scorer's best| per example: {worst}, allowed {BEAM_TOL}"


def test_device_guide_keeps_the_other_slots_nodes_through_a_launch_over_some():
    """The in-flight refill: one slot's prefill rows are processed while the others are in the middle of their sequences.  The node
    buffers swap after every launch, so the launch over some slots must hand the others' nodes on."""
    from llark_amd.m2t.guide import ChoiceSets, DeviceGuide
    V = 64
    table = GR.build_table([SET_A, SET_B])
    g = DeviceGuide(ChoiceSets([SET_A, SET_B]), 4, V, "cuda", EOS)
    assert g.roots == table[4]
    g.admit([0, 1, 2], [0, 1, None])
    x = torch.randn(4, V, generator=torch.Generator().manual_seed(0)).cuda()
    active = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device="cuda")
    g.process(x, state=active)                                     # prefill rows: the nodes stay where admit put them
    assert g.node.cpu().tolist() == [table[4][0], table[4][1], GR.FREE, GR.FREE]
    out = g.process(x, state=active, last=torch.tensor([10, 20, 5, 0], device="cuda"))
    stepped = [GR.step(table, table[4][0], 10, EOS)[0], GR.step(table, table[4][1], 20, EOS)[0], GR.FREE]
    assert g.node.cpu().tolist()[:3] == stepped
    assert torch.equal(out[2], x[2]) and torch.isneginf(out[0]).sum() == V - 2 and torch.isneginf(out[1]).sum() == V - 2
    g.admit([3], [1])
    one = g.process(x[3:], state=torch.ones((4,), dtype=torch.int32, device="cuda"), slot_of_row=[3])
    assert g.node.cpu().tolist() == stepped + [table[4][1]]
    assert sorted((~torch.isneginf(one[0])).nonzero().view(-1).tolist()) == [20, 22]
    g.process(x, last=torch.tensor([11, 21, 7, 22], device="cuda"))
    want = [GR.step(table, stepped[0], 11, EOS)[0], GR.step(table, stepped[1], 21, EOS)[0], GR.FREE, GR.step(table, table[4][1], 22, EOS)[0]]
    assert g.node.cpu().tolist() == want
    g.check()
    g.release([0, 3])
    assert g.node.cpu().tolist() == [GR.FREE, want[1], GR.FREE, GR.FREE]
    g.process(x, last=torch.tensor([0, 9, 0, 0], device="cuda"))  # slot 1 is handed a token outside its set
    with pytest.raises(RuntimeError, match="outside its choice set"):
        g.check()
    g.check(off_set=False)


def test_llama_multinomial_path_with_every_continuation_banned_raises():
    """``torch.multinomial`` cannot draw from a row without a finite logit: such a row draws any token, and the call ends with the
    guide's own message instead of a failed draw."""
    m, kw, rows = _kw("llama_uniform")
    used = {int(t) for r in rows for t in r.tolist()} | {EOS}
    a, g = [t for t in range(3, 60) if t not in used][:2]
    torch.manual_seed(5)
    with pytest.raises(RuntimeError, match="no allowed token left"):
        m.generate(**kw, do_sample=True, temperature=1.0, no_repeat_ngram_size=2, allowed_continuations=[[[a, a, a, a]], [[g]]])


@pytest.mark.parametrize("kind", ["llama", "mpt"])
def test_inflight_composition_with_no_repeat_ngram_size_and_the_error_for_a_row_left_empty(kind):
    """In flight the n-gram ban and the guide compose as in ``generate``; an example whose every continuation is banned ends the run
    with an error when it is released -- its completion is never handed out."""
    from llark_amd.m2t.constraints import TokenConstraints
    from llark_amd.m2t.infer_driver import generate_inflight
    m, tok, ex = CG._inflight_examples(kind)
    V = m.config.vocab_size
    sets, bad_sets, guided = [], [], []
    for i, e in enumerate(ex):
        free = [t for t in range(3, V - 3) if t != EOS and t not in set(e[0].tolist())]
        which = None
        if i % 2 == 0 and len(free) >= 4:
            a, b, c, d = free[:4]
            which = len(sets)
            sets.append([[a, b, a, b, c], [a, b, a, d]])          # (a, b) twice is banned: the second member is the only one left
            bad_sets.append([[a, a, a, a]] if len(guided) == 1 else sets[-1])      # the second guided example: (a, a) twice
            guided.append(i)
        ex[i] = (e[0], e[1], 7, e[3] if len(e) > 3 else None, which)
    assert len(guided) >= 3
    cons = TokenConstraints(no_repeat_ngram_size=2)
    restore = _with_eos(m)
    try:
        got = dict(generate_inflight(m, iter(ex), slots=3, max_new_tokens=7, keywords=(), choice_sets=sets, constraints=cons))
        for i in guided:
            a, b, a2, d = sets[ex[i][4]][1]
            assert got[i][ex[i][0].numel():].tolist() == [a, b, a, d, EOS], f"example {i}: {got[i][ex[i][0].numel():].tolist()}"
        seen = []
        with pytest.raises(RuntimeError, match="no allowed token left .*noticed at the release of example"):
            for item in generate_inflight(m, iter(ex), slots=3, max_new_tokens=7, keywords=(), choice_sets=bad_sets, constraints=cons):
                seen.append(item[0])
        assert guided[1] not in seen, "the example that had no allowed token left was handed out"
    finally:
        restore()
