"""CPU: the order of the stages in llark_amd/m2t/choice.py's TokenChooser, driven with stub parts that record their calls (no GPU, no
``ops`` launch): what ``process`` gets as ``last``, what the choice is made on, what the tracker sees, and who is told to admit, release
and finish."""
import pytest
import torch

from llark_amd.m2t import choice as C

V = 6


class _Cons:
    def __init__(self, log):
        self.log = log

    def admit(self, slots, prompts):
        self.log.append(("cons.admit", list(slots), [p.tolist() for p in prompts]))

    def process(self, logits, state=None, slot_of_row=None, last=None):
        self.log.append(("process", logits, state, None if slot_of_row is None else slot_of_row.tolist(), None if last is None else last.tolist()))
        return logits + 100.0                                       # the processed rows, told apart from the raw ones by their values

    def release(self, slots):
        self.log.append(("cons.release", list(slots)))

    def check(self):
        self.log.append(("cons.check",))


class _Sampler:
    def __init__(self, log, tokens):
        self.log, self.tokens = log, [torch.tensor(t, dtype=torch.int64) for t in tokens]

    def admit(self, slots, prompts, stream_ids):
        self.log.append(("sampler.admit", list(slots), list(stream_ids)))

    def __call__(self, rows, state=None, slot_of_row=None):
        self.log.append(("sample", rows, state, None if slot_of_row is None else slot_of_row.tolist()))
        return self.tokens.pop(0)

    def release(self, slots):
        self.log.append(("sampler.release", list(slots)))


class _Tracker:
    def __init__(self, log):
        self.log = log

    def admit(self, slots):
        self.log.append(("tracker.admit", list(slots)))

    def __call__(self, logits, tokens, state=None, slot_of_row=None):
        self.log.append(("track", logits, tokens.tolist(), state, None if slot_of_row is None else slot_of_row.tolist()))


def _chooser(n_slots, tokens=(), cons=True, sampler=True, tracker=True, choose=None):
    log = []
    ch = C.TokenChooser(n_slots, V, "cpu", choose=choose)
    assert ch.cons is None and ch.sampler is None and ch.tracker is None and ch.last is None       # all off: nothing was constructed
    ch.cons = _Cons(log) if cons else None
    ch.sampler = _Sampler(log, tokens) if sampler else None
    ch.tracker = _Tracker(log) if tracker else None
    return ch, log


def _logits(rows, seed):
    return torch.randn(rows, V, generator=torch.Generator().manual_seed(seed))


def test_prefill_call_then_a_decode_call():
    ch, log = _chooser(2, tokens=[[4, 1], [2, 5]])
    prompts = [torch.tensor([1, 2, 3]), torch.tensor([7])]
    ch.admit([0, 1], prompts)
    assert log == [("cons.admit", [0, 1], [[1, 2, 3], [7]]), ("sampler.admit", [0, 1], [0, 1]), ("tracker.admit", [0, 1])]
    del log[:]
    raw, state = _logits(2, 0), torch.zeros(2, dtype=torch.int32)
    got = ch(raw, state=state)
    assert got.tolist() == [4, 1]
    (p, p_logits, p_state, p_sor, p_last), (s, s_rows, s_state, s_sor), (t, t_logits, t_tokens, t_state, t_sor) = log
    assert (p, s, t) == ("process", "sample", "track")
    assert p_last is None and p_sor is None and p_logits is raw and p_state is state        # a prefill call: nothing is appended
    assert torch.equal(s_rows, raw + 100.0) and s_state is state                             # the choice reads the processed rows
    assert t_logits is raw and t_tokens == [4, 1] and t_state is state                       # the tracker: the RAW logits, the chosen tokens
    del log[:]
    raw2 = _logits(2, 1)
    assert ch(raw2, state=state).tolist() == [2, 5]
    assert log[0][0] == "process" and log[0][1] is raw2 and log[0][4] == [4, 1]              # last: what the first call handed out
    assert log[2][1] is raw2 and log[2][2] == [2, 5]


def test_a_refill_is_a_prefill_call_for_its_slot_only():
    ch, log = _chooser(3, tokens=[[1, 2, 3], [4, 4, 4], [5], [0, 1, 2]])
    ch.admit([0, 1, 2], [torch.tensor([1])] * 3, stream_ids=[10, 11, 12])
    assert ("sampler.admit", [0, 1, 2], [10, 11, 12]) in log
    ch(_logits(3, 0))
    ch(_logits(3, 1))
    del log[:]
    ch.admit([1], [torch.tensor([9, 9])], stream_ids=[13])
    assert ch(_logits(1, 2), slot_of_row=[1]).tolist() == [5]
    process = [e for e in log if e[0] == "process"][0]
    assert process[3] == [1] and process[4] is None                                          # slot 1's prefill rows: nothing appended
    assert [e for e in log if e[0] == "sample"][0][3] == [1] and [e for e in log if e[0] == "track"][0][4] == [1]
    del log[:]
    ch(_logits(3, 3))
    assert log[0][0] == "process" and log[0][3] is None and log[0][4] == [4, 5, 4]           # slot 1: its refill token; the others: theirs


def test_choose_reads_the_processed_rows():
    seen = []

    def choose(rows):
        seen.append(rows)
        return rows.argmax(-1, keepdim=True)
    ch, log = _chooser(2, sampler=False, choose=choose)
    ch.admit([0, 1], [torch.tensor([1]), torch.tensor([2])])
    raw = _logits(2, 4)
    got = ch(raw)
    assert len(seen) == 1 and torch.equal(seen[0], raw + 100.0)
    assert got.shape == (2,) and got.tolist() == raw.argmax(-1).tolist()
    assert [e[0] for e in log if e[0] in ("process", "track")] == ["process", "track"] and log[-1][1] is raw


def test_all_off_builds_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a part was constructed with every stage off")
    for name in ("DeviceConstraints", "DeviceSampler", "LogprobTracker"):
        monkeypatch.setattr(C, name, boom)
    assert C.TokenChooser.build(2, V, "cpu") is None
    assert C.TokenChooser.build(2, V, "cpu", sampling=None, constraints=None, logprobs=False, choose=lambda rows: rows.argmax(-1)) is None
    with pytest.raises(AssertionError, match="a part was constructed"):
        C.TokenChooser.build(2, V, "cpu", logprobs=True, logprob_width=4)


@pytest.mark.parametrize("part", ["cons", "sampler", "tracker"])
def test_release_and_finish_reach_the_parts_that_exist(part):
    ch, log = _chooser(2, cons=part == "cons", sampler=part == "sampler", tracker=part == "tracker")
    ch.release([1])
    ch.finish()
    assert log == {"cons": [("cons.release", [1]), ("cons.check",)], "sampler": [("sampler.release", [1])], "tracker": []}[part]
