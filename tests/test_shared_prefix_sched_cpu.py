"""Shared prompt prefixes in the in-flight scheduler, without a GPU: which examples fork from which slot and at what length, which
get a full prefill, and that outputs, budgets and EOS handling do not change -- against fake backends in the style of
tests/test_inflight_sched_cpu.py (imported, not edited)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_inflight_sched_cpu import EOS, FakeBackend  # noqa: E402

AUDIO_START, AUDIO_END, FRAME = 900, 901, 902
HEADER = list(range(300, 310))
FILL = 5


def _prompt(tag, question, audio_first=True, frames=70):
    """[tag is NOT part of the prompt: the fake's script key is the LAST question token]"""
    audio = [AUDIO_START] + [FRAME] * frames + [AUDIO_END]
    return torch.tensor(HEADER + (audio + question if audio_first else question + audio))


class ForkBackend(FakeBackend):
    """FakeBackend with the fork protocol: a forked slot holds n copied positions until its suffix arrives; the token script of a
    slot is keyed by the last token of its WHOLE prompt (copied prefix + suffix), so a wrong fork length or source changes the output."""
    audio_token_ids = (AUDIO_START, AUDIO_END)

    def __init__(self, n, scripts, filler):
        super().__init__(n, scripts, filler)
        self.forked = {}

    def _next(self, b):
        prompt, gen = self.slots[b]
        sc = self.scripts.get(int(prompt[-1]), [])
        t = sc[len(gen)] if len(gen) < len(sc) else self.filler
        gen.append(t)
        return t

    def fork(self, src, dsts, n):
        self.calls.append(("fork", src, list(dsts), n))
        assert self.slots[src] is not None and src not in self.forked, f"fork from slot {src}, which is not active"
        assert 1 <= n <= len(self.slots[src][0])
        for b in dsts:
            assert self.slots[b] is None and b not in self.forked, f"fork into busy slot {b}"
            self.forked[b] = self.slots[src][0][:n]

    def prefill(self, slots, prompts, encodings, past=None):
        self.calls.append(("prefill", list(slots), None if past is None else list(past)))
        out = []
        for i, (b, p) in enumerate(zip(slots, prompts)):
            assert self.slots[b] is None, f"slot {b} prefilled while busy"
            if past is not None and past[i] > 0:
                assert encodings[i] is None and len(self.forked[b]) == past[i], f"slot {b}: suffix at {past[i]} without a fork to that length"
                assert not any(t in self.audio_token_ids for t in p.tolist()), "audio token in a suffix"
                self.slots[b] = (self.forked.pop(b) + p.tolist(), [])
            else:
                assert b not in self.forked
                self.slots[b] = (p.tolist(), [])
            out.append(self._next(b))
        return out


def _run(backend, examples, n_slots, share, budget=4, **kw):
    from llark_amd.m2t.infer_driver import InflightScheduler
    sched = InflightScheduler(backend, n_slots, budget, EOS, None, share_prefix=share, **kw)
    outs = dict(sched.run(iter(examples)))
    return {i: t.tolist() for i, t in outs.items()}, sched.trace


def _examples():
    """clip A: three audio-first questions; clip B: two audio-LAST questions; clip C: two identical prompts; one example without key"""
    q = lambda *t: list(t)
    return [(_prompt("A", q(11, 12, 13)), "encA", None, "A"), (_prompt("A", q(11, 14)), "encA", None, "A"),
            (_prompt("A", q(15, 16, 17, 18)), "encA", None, "A"),
            (_prompt("B", q(21, 22), audio_first=False), "encB", None, "B"), (_prompt("B", q(21, 23), audio_first=False), "encB", None, "B"),
            (_prompt("C", q(31, 32)), "encC", None, "C"), (_prompt("C", q(31, 32)), "encC", None, "C"),
            (_prompt("D", q(41)), "encD", 2)]


SCRIPTS = {13: [7, 7, 7, 7], 14: [8, EOS], 18: [9, 9, 9, 9], 22: [6, 6, 6, 6], 23: [6, 6, 6, 6], 32: [4, 4, 4, 4], 41: [3, 3, 3]}
PRE = len(HEADER) + 72                               # header + <audio_start> + 70 frames + <audio_end>


def test_fork_decisions_lengths_and_outputs():
    ex = _examples()
    off, trace_off = _run(ForkBackend(8, SCRIPTS, FILL), ex, 8, share=False)
    be = ForkBackend(8, SCRIPTS, FILL)
    on, trace = _run(be, ex, 8, share=True)
    assert on == off                                                         # outputs, budgets, EOS: unchanged
    assert on[1][-2:] == [8, EOS] and len(on[7]) == len(ex[7][0]) + 2 and len(on[0]) == len(ex[0][0]) + 4
    forks = [e for e in trace if e[0] == "fork"]
    # same-round siblings: the first of a clip in full, the others fork from it.  A: common prefix = header + audio block + token 11
    # for example 1 (PRE + 1), the block alone for example 2 (PRE); identical prompts (C) fork at len - 1; audio-last siblings (B) share
    # only the header + one question token: below min_shared -> full prefill
    assert forks == [("fork", 0, 1, PRE + 1), ("fork", 0, 2, PRE), ("fork", 5, 6, len(ex[6][0]) - 1)]
    prefills = [e for e in trace if e[0] == "prefill"]
    assert prefills[0] == ("prefill", (0, 3, 4, 5, 7), (0, 3, 4, 5, 7)) and prefills[1] == ("prefill", (1, 2, 6), (1, 2, 6))
    assert be.calls[:5] == [("prefill", [0, 3, 4, 5, 7], None), ("fork", 0, [1], PRE + 1), ("fork", 0, [2], PRE), ("fork", 5, [6], len(ex[6][0]) - 1),
                            ("prefill", [1, 2, 6], [PRE + 1, PRE, len(ex[6][0]) - 1])]
    assert be.slots == [None] * 8 and be.forked == {}


def test_audio_last_siblings_never_fork_even_with_a_small_threshold():
    """audio last: the common prefix ends inside the question, the rest holds the audio block -> refused whatever min_shared is"""
    ex = _examples()[3:5]
    be = ForkBackend(4, SCRIPTS, FILL)
    _, trace = _run(be, ex, 4, share=True, min_shared=1)
    assert [e for e in trace if e[0] == "fork"] == [] and be.calls[0] == ("prefill", [0, 1], None)


def test_sibling_after_its_lineage_finished_gets_a_full_prefill():
    """one slot: every example finds its clip's slot released; two slots with another clip in between: the same"""
    a0, a1 = _examples()[:2]
    be = ForkBackend(1, SCRIPTS, FILL)
    on, trace = _run(be, [a0, a1], 1, share=True)
    assert [e for e in trace if e[0] == "fork"] == [] and all(c[2] is None for c in be.calls if c[0] == "prefill")
    off, _ = _run(ForkBackend(1, SCRIPTS, FILL), [a0, a1], 1, share=False)
    assert on == off


def test_late_sibling_forks_from_an_active_slot():
    """budget 2 for the first example of clip C, 6 for the second: when the third arrives (slot 0 refilled), slot 1 is the source"""
    c = _examples()[5]
    ex = [(c[0], "encC", 2, "C"), (c[0], "encC", 6, "C"), (c[0], "encC", 2, "C")]
    be = ForkBackend(2, SCRIPTS, FILL)
    on, trace = _run(be, ex, 2, share=True, budget=6)
    n = len(c[0]) - 1
    assert [e for e in trace if e[0] == "fork"] == [("fork", 0, 1, n), ("fork", 1, 0, n)]
    off, _ = _run(ForkBackend(2, SCRIPTS, FILL), ex, 2, share=False, budget=6)
    assert on == off


def test_backend_without_fork_and_flag_off_are_todays_scheduler():
    from llark_amd.m2t.infer_driver import InflightScheduler
    ex = _examples()
    scripts = {int(e[0][0]): [4, 4, EOS] for e in ex}                        # FakeBackend keys scripts by the first prompt token
    plain = FakeBackend(3, scripts, FILL)
    s0 = InflightScheduler(plain, 3, 4, EOS, None)
    want = {i: t.tolist() for i, t in s0.run(iter([e[:3] for e in ex]))}
    for share, backend in ((True, FakeBackend(3, scripts, FILL)), (False, FakeBackend(3, scripts, FILL))):
        s = InflightScheduler(backend, 3, 4, EOS, None, share_prefix=share)      # no fork method: full prefills only
        got = {i: t.tolist() for i, t in s.run(iter(ex))}
        assert got == want and s.trace == s0.trace and backend.calls == plain.calls
    # a backend WITH fork, flag off: the same trace, no fork call, no `past` argument
    be = ForkBackend(3, SCRIPTS, FILL)
    _, trace = _run(be, ex, 3, share=False)
    be_ref = ForkBackend(3, SCRIPTS, FILL)
    _, trace_ref = _run(be_ref, [e[:3] for e in ex], 3, share=False)
    assert trace == trace_ref and all(c[0] != "fork" and (c[0] != "prefill" or c[2] is None) for c in be.calls)


def test_generate_inflight_passes_the_flag():
    """generate_inflight(share_prefix=True) on a model whose slot backend forks"""
    from llark_amd.m2t.infer_driver import generate_inflight

    class M:
        generation_config = type("GC", (), {"eos_token_id": EOS})()

        def slot_backend(self, n):
            self.be = ForkBackend(n, SCRIPTS, FILL)
            return self.be

    m, trace = M(), []
    ex = _examples()[:3]
    got = dict(generate_inflight(m, iter(ex), slots=3, max_new_tokens=4, keywords=(), trace=trace, share_prefix=True))
    assert [e for e in trace if e[0] == "fork"] == [("fork", 0, 1, PRE + 1), ("fork", 0, 2, PRE)]
    m2, trace2 = M(), []
    got2 = dict(generate_inflight(m2, iter(ex), slots=3, max_new_tokens=4, keywords=(), trace=trace2))
    assert not any(e[0] == "fork" for e in trace2) and {i: t.tolist() for i, t in got.items()} == {i: t.tolist() for i, t in got2.items()}
