"""CPU: the float64 reference of tests/logprob_ref.py against known answers and torch.log_softmax, and its skip / history rules."""
import math

import numpy as np
import torch

import logprob_ref as R


def test_known_answers():
    for V in (1, 7, 1025):
        lp, rk, E = R.row_logprob(np.full(V, 2.5, dtype=np.float32), V // 2)
        assert abs(lp + math.log(V)) < 1e-12 and rk == 0 and E == 0.0
    # k tokens at a, the other V - k at b < a: log p(a-token) = -log(k + (V - k) exp(b - a))
    V, k, a, b = 100, 3, 4.0, 1.0
    row = np.full(V, b, dtype=np.float32)
    row[[5, 50, 99]] = a
    z = k + (V - k) * math.exp(b - a)
    lp, rk, E = R.row_logprob(row, 50)
    assert abs(lp + math.log(z)) < 1e-12 and rk == 0
    lp, rk, E = R.row_logprob(row, 51)
    assert abs(lp - ((b - a) - math.log(z))) < 1e-12 and rk == k
    assert abs(E - (V - k) * math.exp(b - a) * (a - b) / z) < 1e-12


def test_infinities_and_nan():
    row = np.array([0.0, -np.inf, 1.0, -np.inf], dtype=np.float32)
    lp, rk, _ = R.row_logprob(row, 2)
    assert abs(lp + math.log(1 + math.exp(-1))) < 1e-12 and rk == 0
    lp, rk, _ = R.row_logprob(row, 1)
    assert lp == -np.inf and rk == 2
    for bad in ([0.0, np.nan, 1.0], [0.0, np.inf, 1.0], [-np.inf, -np.inf]):
        lp, rk, _ = R.row_logprob(np.array(bad, dtype=np.float32), 0)
        assert math.isnan(lp) and rk == -1


def test_agrees_with_torch_log_softmax_in_float64():
    for V in (63, 1025, 32003):
        rows = R.make_rows(V, 3)
        want = torch.log_softmax(torch.from_numpy(rows).double(), dim=-1).numpy()
        for r in range(3):
            for t in (0, V - 1, int(rows[r].argmax()), V // 3):
                lp, rk, _ = R.row_logprob(rows[r], t)
                assert abs(lp - want[r, t]) <= 1e-12 * max(1.0, abs(lp))
                assert rk == int((rows[r] > rows[r, t]).sum())
                assert 0 < R.tol_of(rows[r], t) < 1e-4


def test_depth_counts_the_kernels_additions():
    assert R.depth(1) == 22 and R.depth(1024) == 22 and R.depth(1025) == 23 and R.depth(32003) == 53 and R.depth(50435) == 71


def test_skip_rules_and_history():
    V, slots, width = 9, 5, 2
    logits = R.make_rows(V, 6)
    sor = [3, 0, 4, 7, 1, 2]                                   # row 3: slot out of range
    state = [R.ROW_ACTIVE, R.ROW_IDLE, R.ROW_ACTIVE, R.ROW_ACTIVE, R.ROW_FINISHED]     # rows 4 (slot 1) and 2 (slot 4) are skipped
    tokens = [2, -1, 5, 1, 0, V]                               # rows 1 and 5: no target
    lp = np.full(6, 9.0)
    rk = np.full(6, -7)
    hist = np.full((slots, width), 9.0)
    count = np.array([0, 0, 0, 2, 0])                          # slot 3 is full already
    total = np.zeros(slots)
    done = R.token_logprob_rows(logits, V, tokens, slots, state, sor, lp, rk, hist, count, total)
    assert done == [0]
    assert lp[1:].tolist() == [9.0] * 5 and rk[1:].tolist() == [-7] * 5
    assert (hist == 9.0).all() and count.tolist() == [0, 0, 0, 3, 0] and total[3] == lp[0] and lp[0] < 0
    # identity slots, two launches accumulate
    count[:] = 0
    total[:] = 0
    for _ in range(3):
        R.token_logprob_rows(logits[:5], V, [1] * 5, slots, logprob=lp, hist=hist, count=count, total=total)
    assert count.tolist() == [3] * 5 and np.allclose(total, 3 * lp[:5]) and np.array_equal(hist[:, 0], lp[:5]) and np.array_equal(hist[:, 1], lp[:5])
