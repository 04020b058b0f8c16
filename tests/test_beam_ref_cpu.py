"""beam_ref (the float64 restatement of the beam step that the GPU tests compare against) on hand-worked cases: the reference has to be
right before anything is measured against it.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402


def logits_of(probs):
    """A logits row whose softmax is `probs`."""
    return np.log(np.asarray(probs, dtype=np.float64))


def lp(p):
    return math.log(p)


def test_two_beams_five_tokens_by_hand():
    """B = 2, V = 5, no eos, prompt of 3 tokens.  Step 0: p = (.1, .4, .3, .15, .05) -> beams (token 1, ln .4), (token 2, ln .3): both
    children of slot 0, so the second moves to slot 1: one copy (0 -> 1).  Step 1: after token 1 p = (.5, .2, .1, .1, .1), after token 2
    p = (.05, .05, .8, .05, .05): candidates .4 * .5 = .20, .3 * .8 = .24, .4 * .2 = .08 -> beams (2, 2) then (1, 0); each parent keeps
    its slot, nothing is copied, and slot 1 now holds rank 0."""
    rows = {(): [.1, .4, .3, .15, .05], (1,): [.5, .2, .1, .1, .1], (2,): [.05, .05, .8, .05, .05]}
    ref = R.BeamRef([3], 2)
    nxt, pairs = ref.step(np.stack([logits_of(rows[()])] * 2))
    assert nxt.tolist() == [1, 2] and pairs == [[(0, 1)]] and ref.rank_of_slot.tolist() == [0, 1]
    assert ref.score == pytest.approx([lp(.4), lp(.3)], rel=1e-6)
    nxt, pairs = ref.step(np.stack([logits_of(rows[(1,)]), logits_of(rows[(2,)])]))
    assert nxt.tolist() == [0, 2] and pairs == [[]] and ref.rank_of_slot.tolist() == [1, 0]
    assert ref.score == pytest.approx([lp(.4 * .5), lp(.3 * .8)], rel=1e-6)
    assert ref.tokens_of_slot(0) == [1, 0] and ref.tokens_of_slot(1) == [2, 2] and ref.cur_len == [5]
    hyps = ref.finalize(2)[0]
    assert [h["tokens"] for h in hyps] == [[2, 2], [1, 0]]
    assert hyps[0]["score"] == pytest.approx(lp(.24) / 5, rel=1e-6) and hyps[0]["length"] == 5 and not hyps[0]["eos"]


def test_eos_below_and_above_rank_b():
    """B = 2, eos = 0.  p = (.35, .3, .2, .1, .05): the eos is candidate 0 (< B): a hypothesis of length = the prompt's 4, sum ln .35;
    the live beams are tokens 1 and 2.  Then rows in which eos is only the 3rd / 4th best candidate of the merged list (>= B): skipped."""
    ref = R.BeamRef([4], 2, eos=0)
    ref.step(np.stack([logits_of([.35, .3, .2, .1, .05])] * 2))
    assert len(ref.heaps[0]) == 1 and ref.heaps[0][0]["length"] == 4 and ref.heaps[0][0]["end_step"] == 0
    assert ref.heaps[0][0]["sum"] == pytest.approx(lp(.35), rel=1e-6) and ref.heaps[0][0]["score"] == pytest.approx(lp(.35) / 4, rel=1e-6)
    assert [ref.tokens_of_slot(s) for s in (0, 1)] == [[1], [2]] and not ref.done[0]
    # merged order: .3 * .5 (tok 3), .2 * .6 (tok 4), .3 * .3 (eos, place 2 >= B: skipped), ...
    nxt, _ = ref.step(np.stack([logits_of([.3, .1, .05, .5, .05]), logits_of([.2, .1, .05, .05, .6])]))
    assert len(ref.heaps[0]) == 1 and sorted(nxt.tolist()) == [3, 4]
    hyps = ref.finalize(2)[0]
    # the live beams join at the end: [1, 3] (ln .15 / 6) beats the early eos (ln .35 / 4)? -1.897 / 6 = -.316 > -1.05 / 4 = -.262: no
    assert hyps[0]["tokens"] == [] and hyps[0]["eos"] and hyps[0]["logprobs"] == pytest.approx([lp(.35)])
    assert hyps[1]["tokens"] == [1, 3] and hyps[1]["score"] == pytest.approx(lp(.15) / 6, rel=1e-6)


def test_heap_eviction_and_done_without_early_stopping():
    """B = 2, eos = 0, length_penalty 1, prompt 2.  Steps that each close one hypothesis at place < B; the third one is better than the
    worst of the two kept and evicts it.  done needs worst >= best candidate / cur_len."""
    ref = R.BeamRef([2], 2, eos=0)
    ref.step(np.stack([logits_of([.02, .5, .46, .01, .01])] * 2))            # eos is 3rd: nothing closes
    assert ref.heaps[0] == []
    ref.step(np.stack([logits_of([.6, .3, .05, .03, .02]), logits_of([.05, .05, .05, .05, .8])]))
    # merged: .46 * .8 = .368 (tok 4), .5 * .6 = .30 (eos, place 1 < 2): closes [1] with sum ln .3, length 3
    assert len(ref.heaps[0]) == 1 and ref.heaps[0][0]["sum"] == pytest.approx(lp(.30), rel=1e-6) and ref.heaps[0][0]["length"] == 3
    assert not ref.done[0]
    live = {tuple(ref.tokens_of_slot(s)): s for s in (0, 1)}
    assert set(live) == {(2, 4), (1, 1)}
    rows = [None, None]
    rows[live[(2, 4)]] = logits_of([.9, .025, .025, .025, .025])              # .368 * .9 = .331: eos at place 0
    rows[live[(1, 1)]] = logits_of([.7, .1, .1, .05, .05])                    # .15 * .7 = .105: eos at place 1
    ref.step(np.stack(rows))
    h = sorted(ref.heaps[0], key=lambda x: -x["score"])
    # three hypotheses arrived: ln .3 / 3 = -.401, ln .331 / 4 = -.276, ln .105 / 4 = -.563 (refused: not above the worst, -.401)
    assert [x["sum"] for x in h] == pytest.approx([lp(.3312), lp(.30)], rel=1e-4) and ref.arrivals[0] == 3
    # best candidate / cur_len = ln .3312 / 4 = -.276 > worst -.401: not done
    assert not ref.done[0]
    # now a weak step: the best candidate is far below the worst hypothesis -> done
    ref2 = R.BeamRef([2], 2, eos=0)
    ref2.heaps[0] = [dict(score=np.float32(-.1), sum=np.float32(-.2), length=2, end_step=0, end_slot=0, arrival=0, eos_lp=-.2),
                     dict(score=np.float32(-.2), sum=np.float32(-.4), length=2, end_step=0, end_slot=0, arrival=1, eos_lp=-.4)]
    ref2.arrivals[0] = 2
    nxt, pairs = ref2.step(np.stack([logits_of([.01, .3, .3, .2, .19])] * 2))    # best = ln .3 / 2 = -.6 < worst -.2
    assert ref2.done[0] and nxt.tolist() == [0, 0] and pairs == [[]] and (ref2.state == R.ROW_FINISHED).all()
    nxt, pairs = ref2.step(np.stack([logits_of([.2] * 5)] * 2))
    assert nxt.tolist() == [0, 0] and ref2.cur_len == [3]                    # a done example stands still


def test_eviction_replaces_the_worst():
    ref = R.BeamRef([1], 2, eos=0)
    for total in (-3.0, -2.0, -1.0, -2.5):
        ref.add(0, total, 1, 0, 0, total)
    assert sorted(float(h["sum"]) for h in ref.heaps[0]) == [-2.0, -1.0] and float(ref.worst(0)) == -2.0 and ref.arrivals[0] == 4


def test_early_stopping_is_done_as_soon_as_the_heap_is_full():
    rows = np.stack([logits_of([.45, .3, .15, .05, .05])] * 2)
    for early, want in ((True, True), (False, False)):
        ref = R.BeamRef([2], 2, eos=0, early_stopping=early)
        ref.heaps[0] = [dict(score=np.float32(-9.0), sum=np.float32(-18.0), length=2, end_step=0, end_slot=0, arrival=0, eos_lp=-1.0)]
        ref.arrivals[0] = 1
        ref.step(rows)                                                       # eos at place 0: the heap is full now; worst = -9
        assert len(ref.heaps[0]) == 2 and ref.done[0] is want                # best / cur_len = ln .45 / 2 = -.4 > -9: only early stops


def test_one_beam_without_eos_is_greedy():
    rng = np.random.default_rng(5)
    table = rng.standard_normal((7, 7)) * 3

    def row_of(e, toks):
        return table[toks[-1] if toks else 3]

    ref, hyps = R.beam_search(row_of, [4], 1, 6)
    greedy, t = [], 3
    for _ in range(6):
        t = int(np.argmax(table[t]))
        greedy.append(t)
    assert hyps[0][0]["tokens"] == greedy and all(p == [] for p in [ref.step(np.stack([table[0]]))[1][0]])


@pytest.mark.parametrize("length_penalty", [1.0, 0.0, 2.0])
def test_score_is_the_backtracked_sum_over_length_to_the_penalty(length_penalty):
    rng = np.random.default_rng(11)
    table = rng.standard_normal((2, 9, 9)) * 2

    def row_of(e, toks):
        return table[e, toks[-1] if toks else 0]

    ref, hyps = R.beam_search(row_of, [3, 5], 3, 7, eos=4, length_penalty=length_penalty, num_return_sequences=3)
    seen_eos = False
    for e, hs in enumerate(hyps):
        assert [float(h["score"]) for h in hs] == sorted((float(h["score"]) for h in hs), reverse=True)
        for h in hs:
            seen_eos |= h["eos"]
            assert len(h["logprobs"]) == len(h["tokens"]) + (1 if h["eos"] else 0) and 4 not in h["tokens"]
            assert h["length"] == [3, 5][e] + len(h["tokens"])
            assert float(h["score"]) == pytest.approx(sum(h["logprobs"]) / h["length"] ** length_penalty, rel=1e-5, abs=1e-6)
    assert seen_eos or length_penalty > 1.0              # a large penalty favours the long, unfinished hypotheses


def test_layout_appends_eos_to_every_short_row():
    """HF's quirk: a row shorter than the width gets eos after its last token whether or not it ended on eos."""
    hyps = [[dict(tokens=[5, 6, 7], logprobs=[-.1, -.2, -.3], eos=False)], [dict(tokens=[8], logprobs=[-.5, -.6], eos=True)],
            [dict(tokens=[9, 9], logprobs=[-.7, -.8], eos=False)]]
    prompts = np.array([[1, 2], [0, 3], [3, 3]])
    ids, lps = R.layout(prompts, hyps, eos=4, pad=0, max_new_tokens=8)
    assert ids.tolist() == [[1, 2, 5, 6, 7, 4], [0, 3, 8, 4, 0, 0], [3, 3, 9, 9, 4, 0]]
    want = np.array([[-.1, -.2, -.3, np.nan], [-.5, -.6, np.nan, np.nan], [-.7, -.8, np.nan, np.nan]])
    np.testing.assert_array_equal(np.isnan(lps), np.isnan(want))
    np.testing.assert_allclose(np.nan_to_num(lps), np.nan_to_num(want))
    ids, _ = R.layout(prompts, hyps, eos=4, pad=0, max_new_tokens=3)          # width capped at S + max_new_tokens: no room for the eos
    assert ids.tolist() == [[1, 2, 5, 6, 7], [0, 3, 8, 4, 0], [3, 3, 9, 9, 4]]


def test_tie_rule_rank_then_token():
    """Identical rows under equal beam scores: the order is rank ascending, then token ascending."""
    ref = R.BeamRef([2], 2)
    ref.score[:] = 0.0
    ref.rank_of_slot[:] = [1, 0]                                             # slot 1 holds rank 0
    nxt, pairs = ref.step(np.stack([logits_of([.3, .3, .2, .1, .1])] * 2))
    # candidates ln .3 four times: (rank 0, tok 0), (rank 0, tok 1), (rank 1, tok 0), ...: both live beams are children of slot 1
    assert ref.trellis[0][0].tolist() == [1, 1] and nxt[1] == 0 and nxt[0] == 1 and pairs == [[(1, 0)]]
    assert ref.rank_of_slot.tolist() == [1, 0]
    c, t, _ = R.row_candidates(logits_of([.2, .3, .3, .1, .1]), 0.0, 2)
    assert t.tolist() == [1, 2, 0, 3]


def test_nan_row_gives_no_candidates():
    c, t, l = R.row_candidates([0.0, np.nan, 1.0, 2.0], 0.0, 1)
    assert t.tolist() == [-1, -1] and np.isinf(c).all()
    ref = R.BeamRef([2], 1)
    ref.step(np.array([[0.0, np.inf, 1.0, 2.0]]))
    assert ref.done[0]
