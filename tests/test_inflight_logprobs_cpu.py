"""The in-flight scheduler's log-probability protocol without a GPU: a fake backend that records its calls.

``take_logprobs(finished)`` must come just before ``release(finished)`` with the same slots, in finish order; the yielded triple
carries one value per generated token (the EOS token included) for budgets and stops at different steps; with the flag off the fake
backend of tests/test_inflight_sched_cpu.py -- which has no ``take_logprobs`` and takes no new keyword -- sees what it always saw."""
import pytest
import torch

from test_inflight_sched_cpu import EOS, FakeBackend, FakeModel

FILLER = 9


class LogprobBackend(FakeBackend):
    """The k-th token of the example whose prompt starts with p gets the 'log-probability' -(p + k / 100)."""

    def __init__(self, n, scripts, filler):
        super().__init__(n, scripts, filler)
        self.lp = [None] * n

    def prefill(self, slots, prompts, encodings):
        for b, p in zip(slots, prompts):
            self.lp[b] = [-float(p[0])]
        return super().prefill(slots, prompts, encodings)

    def decode(self):
        for b in range(self.n):
            if self.slots[b] is not None:
                self.lp[b].append(-(self.slots[b][0][0] + len(self.lp[b]) / 100.0))
        return super().decode()

    def take_logprobs(self, slots):
        self.calls.append(("take", list(slots)))
        for b in slots:
            assert self.slots[b] is not None, f"take_logprobs of slot {b} after its release"
        return [torch.tensor(self.lp[b]) for b in slots]

    def release(self, slots):
        self.calls.append(("release", list(slots)))
        super().release(slots)


def _examples():
    # prompt[0] keys the script; budgets and EOS positions differ: generated lengths 3 (EOS), 2 (budget), 1 (EOS at once), 5, 4 (budget)
    scripts = {10: [5, 5, EOS], 11: [5, 5, 5, 5], 12: [EOS], 13: [5, 5, 5, 5, EOS], 14: []}
    examples = [(torch.tensor([10, 1]), None, 8), (torch.tensor([11, 1, 1]), None, 2), (torch.tensor([12]), None, 8),
                (torch.tensor([13, 1]), None, 8), (torch.tensor([14, 1, 1, 1]), None, 4)]
    return scripts, examples, [3, 2, 1, 5, 4]


def test_take_logprobs_comes_before_release_and_lengths_are_right():
    from llark_amd.m2t.infer_driver import InflightScheduler
    scripts, examples, n_gen = _examples()
    be = LogprobBackend(2, scripts, FILLER)
    sched = InflightScheduler(be, 2, max_new_tokens=8, eos=EOS, logprobs=True)
    outs = list(sched.run(examples))
    assert sorted(o[0] for o in outs) == list(range(5))
    for idx, ids, lp in outs:
        prompt = examples[idx][0]
        assert ids.numel() - prompt.numel() == n_gen[idx] == lp.numel() and lp.dtype == torch.float32
        want = torch.tensor([-(float(prompt[0]) + k / 100.0) for k in range(n_gen[idx])])
        assert torch.equal(lp, want), (idx, lp, want)
    # every take is followed at once by the release of the same slots; the done events list them in the same (finish) order
    takes = [i for i, c in enumerate(be.calls) if c[0] == "take"]
    assert len(takes) == len([c for c in be.calls if c[0] == "release"]) and takes
    for i in takes:
        assert be.calls[i + 1] == ("release", be.calls[i][1])
    done = [ev[1] for ev in sched.trace if ev[0] == "done"]
    assert [b for i in takes for b in be.calls[i][1]] == done


def test_a_wrong_history_length_is_an_error():
    from llark_amd.m2t.infer_driver import InflightScheduler
    scripts, examples, _ = _examples()

    class Short(LogprobBackend):
        def take_logprobs(self, slots):
            return [torch.zeros(0) for _ in slots]
    with pytest.raises(RuntimeError, match="log-probabilities for"):
        list(InflightScheduler(Short(2, scripts, FILLER), 2, eos=EOS, logprobs=True).run(examples))


def test_flag_off_the_old_fake_backend_sees_no_new_call_and_no_new_keyword():
    from llark_amd.m2t.infer_driver import InflightScheduler, generate_inflight
    scripts, examples, n_gen = _examples()
    be = FakeBackend(2, scripts, FILLER)                      # no take_logprobs; prefill takes exactly (slots, prompts, encodings)
    outs = list(InflightScheduler(be, 2, max_new_tokens=8, eos=EOS).run(examples))
    assert all(len(o) == 2 for o in outs) and {c[0] for c in be.calls} == {"prefill", "decode"}
    model = FakeModel(scripts, FILLER)
    outs = dict(generate_inflight(model, examples, slots=2, max_new_tokens=8, keywords=()))
    assert [outs[i].numel() - examples[i][0].numel() for i in range(5)] == n_gen
    assert {c[0] for c in model.backends[0].calls} == {"prefill", "decode"}
    # a model that brings its own backend refuses the flag by name
    with pytest.raises(ValueError, match="return_logprobs"):
        list(generate_inflight(model, examples, slots=2, keywords=(), return_logprobs=True))
