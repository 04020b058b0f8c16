"""CPU: the numpy reference of the device sampler (tests/sample_ref.py) -- Philox known answers, agreement with the logits
processors of transformers, and the cap on ambiguous rows that the GPU tests rely on."""
import numpy as np
import pytest

import sample_ref as R


def test_philox4x32_10_known_answers():
    assert ["%08x" % w for w in R.philox4x32_10((0, 0, 0, 0), (0, 0))] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = 0xFFFFFFFF
    assert ["%08x" % w for w in R.philox4x32_10((ones,) * 4, (ones,) * 2)] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    # Random123's third vector (digits of pi): the key schedule and the word order in one
    assert ["%08x" % w for w in R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))] == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_philox_uniform_is_a_24_bit_fraction_of_word0():
    w0 = R.philox4x32_10((7, 0, 5, 1), (3, 2))[0]
    u = R.philox_uniform(seed=(2 << 32) | 3, stream_id=(1 << 32) | 5, draw=7)
    assert u == (w0 >> 8) / 2 ** 24 and 0.0 <= u < 1.0 and np.float32(u) == u
    assert R.philox_uniform(1, 0, 0) != R.philox_uniform(1, 1, 0) != R.philox_uniform(1, 1, 1)


def test_processors_on_a_hand_row():
    row = np.array([2.0, -1.0, 0.5, 2.0, -np.inf, 1.0], dtype=np.float32)
    seen = np.array([1, 1, 0, 0, 0, 0], dtype=bool)
    pen = R.penalise(row, seen, 2.0)
    assert pen.tolist() == [1.0, -2.0, 0.5, 2.0, -np.inf, 1.0] and R.greedy_token(pen) == 3
    ref = R.process(row, seen, top_k=2)                       # the two 2.0 tie at the threshold: both kept, nothing else
    assert ref["keep"].tolist() == [True, False, False, True, False, False] and ref["kept"] == 2 and ref["thresh"] == 2.0
    ref = R.process(row, seen, top_k=3)                       # k-th largest is 1.0
    assert ref["kept"] == 3 and ref["thresh"] == 1.0
    ref = R.process(row, seen, top_p=0.5)                     # mass above the tied maxima is 0 < p Z: both stay; 1.0 sees 2 of 2.63 Z above
    assert ref["keep"].tolist() == [True, False, False, True, False, False]
    tok, ok, zk, _ = R.draw(ref["l"], ref["e"], ref["keep"], 0.5)
    assert zk == 2.0 and tok == 3 and R.draw(ref["l"], ref["e"], ref["keep"], 0.49)[0] == 0
    assert R.process(np.array([np.nan, 1.0], dtype=np.float32), np.zeros(2, bool)) == {"fallback": 0}
    assert R.process(np.full(3, -np.inf, dtype=np.float32), np.zeros(3, bool)) == {"fallback": 0}
    assert R.process(np.array([0.0, np.inf], dtype=np.float32), np.zeros(2, bool)) == {"fallback": 1}


def test_pack_seen_bit_layout():
    seen = np.zeros((2, 70), dtype=bool)
    seen[0, [0, 31, 32, 69]] = True
    seen[1, 33] = True
    w = R.pack_seen(seen).view(np.uint32)
    assert w.shape == (2, 3) and w[0].tolist() == [0x80000001, 1, 1 << 5] and w[1].tolist() == [0, 2, 0]


@pytest.mark.parametrize("name", list(R.PARAM_SETS))
def test_kept_set_equals_the_transformers_processors(name):
    """RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on tie-free rows.  The
    warpers work in fp32: a row whose top-p boundary lies within 1e-5 of p in the reference is not compared (none may be needed)."""
    torch = pytest.importorskip("torch")
    try:
        from transformers import RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    except Exception as e:                                    # noqa: BLE001 -- the classes moved between releases
        pytest.skip(f"transformers' logits processors do not import: {e}")
    params = R.PARAM_SETS[name]
    logits, seen, _ = R.make_case(1025, 16, seed=3)
    compared = 0
    for r in range(logits.shape[0]):
        ref = R.process(logits[r], seen[r], **params)
        p = float(np.float32(params.get("top_p", 1.0)))
        edge = np.abs(ref["above"][ref["in_k"]] / ref["Z"] - p).min() if p < 1 else 1.0
        if edge < 1e-5 or np.unique(ref["l"]).size != ref["l"].size:
            continue
        scores = torch.from_numpy(logits[r: r + 1].copy())
        ids = torch.from_numpy(np.flatnonzero(seen[r]))[None]
        if params.get("theta", 1.0) != 1.0:
            scores = RepetitionPenaltyLogitsProcessor(params["theta"])(ids, scores)
        if params.get("temperature", 1.0) != 1.0:
            scores = TemperatureLogitsWarper(params["temperature"])(ids, scores)
            assert np.array_equal(scores[0].numpy(), ref["l"])                       # steps 1-2 are bit-exact
        if params.get("top_k", 0):
            scores = TopKLogitsWarper(params["top_k"])(ids, scores)
        if p < 1:
            scores = TopPLogitsWarper(p)(ids, scores)
        assert np.array_equal(torch.isfinite(scores[0]).numpy(), ref["keep"]), (name, r)
        compared += 1
    assert compared >= 12


@pytest.mark.parametrize("vocab", R.VOCABS)
def test_reference_alone_stays_inside_the_ambiguity_cap(vocab):
    """The GPU draw test lets a row with more than one acceptable token pass on any of them, and fails a case with more than 1/8 of
    its rows ambiguous.  The inputs must not loosen that: on this family the reference itself leaves at most 1/8 of 64 rows
    ambiguous under the tolerance tests/sample_ref.py derives (C_TOL = 96), for every parameter set."""
    rows = 64
    logits, seen, u = R.make_case(vocab, rows)
    for name, params in R.PARAM_SETS.items():
        n = R.ambiguous_rows(logits, seen, u, **params)
        print(f"vocab {vocab} {name}: {n} of {rows} rows ambiguous at c = {R.C_TOL:g}")
        assert n <= rows // 8, (vocab, name, n)
