"""CPU: SamplingParams refuses bad values by name, generate()'s arguments map to the device sampler only when they ask for it, and the
in-flight scheduler hands example indices and whole prompts to its backend only when sampling is on."""
import pytest
import torch

from llark_amd.m2t.infer_driver import InflightScheduler
from llark_amd.m2t.sampling import SamplingParams, params_from_generate


@pytest.mark.parametrize("field,bad", [("temperature", 0.0), ("temperature", -1.0), ("temperature", float("nan")), ("temperature", "hot"),
                                       ("top_k", -1), ("top_k", 2.5), ("top_p", 0.0), ("top_p", 1.01), ("top_p", float("inf")),
                                       ("repetition_penalty", 0.0), ("repetition_penalty", -1.3), ("seed", 1.5), ("seed", 2 ** 64)])
def test_sampling_params_name_the_bad_value(field, bad):
    with pytest.raises(ValueError, match=field):
        SamplingParams(**{field: bad})


def test_params_from_generate():
    assert params_from_generate(True, 0.8, None, None, None, None) is None              # Llama's torch path: temperature only, no seed
    assert params_from_generate(False, 1.0, 50, 0.9, None, 3) is None                    # greedy ignores the warpers, as HF does
    assert params_from_generate(True, 0.8, None, None, None, None, always=True) == SamplingParams(True, 0.8)
    assert params_from_generate(True, 0.8, 50, None, None, None) == SamplingParams(True, 0.8, 50, 1.0, 1.0, 0)
    assert params_from_generate(True, 1.0, None, None, None, 7) == SamplingParams(True, seed=7)
    assert params_from_generate(False, 1.0, None, None, 1.3, None) == SamplingParams(False, repetition_penalty=1.3)
    assert params_from_generate(False, 1.0, None, None, 1.0, None) is None
    with pytest.raises(ValueError, match="top_p"):
        params_from_generate(False, 1.0, None, 2.0, None, None)
    assert SamplingParams(seed=2 ** 64 - 1).seed == 2 ** 64 - 1 and not SamplingParams().active


class _Backend:
    """Every example answers 7 7 7 ...; records how prefill was called."""
    audio_token_ids = ()

    def __init__(self, n):
        self.n, self.calls, self.busy = n, [], set()

    def prefill(self, slots, prompts, encodings, past=None, **kw):
        self.calls.append((tuple(slots), [p.tolist() for p in prompts], past, kw))
        self.busy |= set(slots)
        return [7] * len(slots)

    def fork(self, src, dsts, n):
        self.calls.append(("fork", src, tuple(dsts), n))

    def decode(self):
        return [7] * self.n

    def release(self, slots):
        self.busy -= set(slots)


def _examples():
    head = list(range(100, 170))
    return [(torch.tensor(head + [5, 6]), None, 2, "clip"), (torch.tensor(head + [8]), None, 2, "clip"), (torch.tensor([1, 2, 3]), None, 2, "other")]


def test_scheduler_passes_indices_and_whole_prompts_only_when_sampling():
    be = _Backend(3)
    out = dict(InflightScheduler(be, 3, 2, None, None, share_prefix=True, sampling=True).run(_examples()))
    assert sorted(out) == [0, 1, 2]
    full, fork, forked = be.calls[0], be.calls[1], be.calls[2]
    assert full[0] == (0, 2) and full[2] is None and full[3]["indices"] == [0, 2] and [w.tolist() for w in full[3]["whole"]] == full[1]
    assert fork == ("fork", 0, (1,), 70)
    assert forked[0] == (1,) and forked[1] == [[8]] and forked[2] == [70] and forked[3]["indices"] == [1]
    assert forked[3]["whole"][0].tolist() == list(range(100, 170)) + [8]                 # the forked slot has seen its whole prompt
    be = _Backend(3)
    dict(InflightScheduler(be, 3, 2, None, None, share_prefix=True).run(_examples()))
    assert [c[3] for c in be.calls if c[0] != "fork"] == [{}, {}]                        # off: the backend's signature is what it was
