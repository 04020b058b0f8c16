"""llark_spec_verify_rows and llark_spec_draft_rows (csrc/speculate.hip) against the plain-Python restatement of tests/spec_ref.py,
exactly: every output word of every slot, the untouched words of idle and finished slots included.  Vocab 97 inside rows of 104
floats (the columns behind the vocabulary hold the row's largest values and must never win), 3 slots, stride 4 and 8."""
import math

import pytest
import torch

import spec_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOCAB, LDL, SLOTS, LD_HIST = 97, 104, 3, 24
PAD, EOS = 96, 11
NAN, INF = float("nan"), float("inf")


def _ops():
    from llark_amd import ops
    return ops


def _logits(stride, rows):
    """rows: {(slot, i): {index: value}} on top of a seeded background in (-1, 1); columns >= VOCAB hold +inf"""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(SLOTS * stride, LDL, generator=g) * 2 - 1
    x[:, VOCAB:] = INF
    for (b, i), put in rows.items():
        for j, v in put.items():
            x[b * stride + i, j] = v
    return x


def _run_verify(stride, logits, ids, blk, state, pos, budget, hist):
    ops = _ops()
    i32, i64 = torch.int32, torch.int64
    d = dict(ids=torch.tensor(ids, dtype=i64).view(-1), blk=torch.tensor(blk, dtype=i32), state=torch.tensor(state, dtype=i32),
             pos=torch.tensor(pos, dtype=i32), budget=torch.tensor(budget, dtype=i32), next_ids=torch.full((SLOTS,), -7, dtype=i64),
             hist=torch.full((SLOTS, LD_HIST), -1, dtype=i64), hist_len=torch.tensor([len(h) for h in hist], dtype=i32))
    for b, h in enumerate(hist):
        d["hist"][b, :len(h)] = torch.tensor(h, dtype=i64)
    d = {k: v.to(DEV) for k, v in d.items()}
    buf = ops.spec_step_buffer(SLOTS, DEV)
    buf.fill_(-3)
    out_tokens, n_out = ops.spec_step_views(buf)
    lg = logits.to(DEV)
    ops.spec_verify_rows(lg, d["ids"], d["blk"], d["state"], d["pos"], d["budget"], out_tokens, n_out, d["next_ids"], d["hist"], d["hist_len"],
                         eos=EOS, pad=PAD, vocab=VOCAB)
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu().view(torch.int32), logits.view(torch.int32)), "the logits were modified"
    host = buf.cpu()                                           # ONE transfer carries the tokens and the counts
    toks, n = ops.spec_step_views(host)
    got = {k: v.cpu().tolist() for k, v in d.items()}
    for b in range(SLOTS):
        greedy = [S.argmax(logits[b * stride + i, :VOCAB].tolist()) for i in range(stride)]
        h = list(hist[b])
        want = S.verify(greedy, ids[b], min(blk[b], stride), state[b], pos[b], budget[b], EOS, PAD, h, LD_HIST)
        assert toks[b].tolist() == want[0] and int(n[b]) == want[1], (b, toks[b].tolist(), int(n[b]), want)
        assert (got["state"][b], got["pos"][b], got["budget"][b]) == want[2:5], (b, got, want)
        assert got["next_ids"][b] == (-7 if want[5] is None else want[5]), (b, got["next_ids"], want)
        assert got["hist_len"][b] == len(h) and got["hist"][b][:len(h)] == h and all(t == -1 for t in got["hist"][b][len(h):]), (b, got["hist"][b], h)
    return toks.tolist(), n.tolist(), got


@pytest.mark.parametrize("stride", [4, 8])
def test_verify_accept_reject_partial(stride):
    """slot 0 accepts every draft, slot 1 none, slot 2 a partial run whose later rows match again (they must not count)"""
    win = lambda t: {t: 5.0}
    rows = {}
    ids = [[1] + [20 + i for i in range(stride - 1)], [2] + [30 + i for i in range(stride - 1)], [3] + [40 + i for i in range(stride - 1)]]
    for i in range(stride):
        rows[(0, i)] = win(20 + i)                            # g_i = the next row's input: all accepted, plus the bonus token
        rows[(1, i)] = win(60 + i)                            # never the draft
        rows[(2, i)] = win(40 + i if i != 2 else 77)          # rows 0, 1 match, row 2 does not, row 3.. would again
    toks, n, _ = _run_verify(stride, _logits(stride, rows), ids, [stride] * 3, [S.ACTIVE] * 3, [5, 0, 9], [100] * 3, [[1], [2], [3]])
    assert n == [stride, 1, 3] and toks[2][:3] == [40, 41, 77]


@pytest.mark.parametrize("stride", [4, 8])
def test_verify_eos_budget_and_short_blocks(stride):
    """eos inside the accepted run finishes the slot and drops the rest; a budget smaller than the run cuts it (an eos behind the cut
    does not finish); blk < stride: rows >= blk are never read (they hold NaN rows that would win)"""
    rows = {}
    ids = [[1, 20, EOS, 22] + [PAD] * (stride - 4), [2, 30, 31, 32] + [PAD] * (stride - 4), [3, 40, 41, 42] + [PAD] * (stride - 4)]
    for i, t in enumerate([20, EOS, 22, 23]):
        rows[(0, i)] = {t: 3.0}
    for i, t in enumerate([30, 31, EOS, 33]):
        rows[(1, i)] = {t: 3.0}
    rows[(2, 0)], rows[(2, 1)] = {40: 3.0}, {41: 3.0}
    rows[(2, 2)] = {j: NAN for j in range(LDL)}               # row 2 of a block of 2: not read
    toks, n, got = _run_verify(stride, _logits(stride, rows), ids, [4, 4, 2], [S.ACTIVE] * 3, [5, 6, 7], [100, 2, 100], [[1], [2], [3]])
    assert n == [2, 2, 2] and got["state"] == [S.FINISHED, S.ACTIVE, S.ACTIVE] and got["budget"] == [98, 0, 98]
    assert toks[0][:2] == [20, EOS] and toks[1][:2] == [30, 31] and toks[2][:2] == [40, 41]


@pytest.mark.parametrize("stride", [4, 8])
def test_verify_ties_nan_idle_finished(stride):
    """exact ties take the first maximal index (placed so that they land in different lanes and waves); a NaN row takes its first
    NaN; +-inf; idle and finished slots, a block of 0 rows and an empty budget leave every word of the slot as it was"""
    rows = {(0, 0): {70: 2.5, 6: 2.5, 69: 2.5}, (0, 1): {50: NAN, 13: NAN, 96: INF}, (0, 2): {j: -INF for j in range(VOCAB)},
            (0, 3): {96: INF, 64: INF, 0: 1e30}}
    ids = [[1, 6, 13, 0] + [PAD] * (stride - 4), [2, 3, 4, 5] + [PAD] * (stride - 4), [3, 4, 5, 6] + [PAD] * (stride - 4)]
    toks, n, _ = _run_verify(stride, _logits(stride, rows), ids, [4, 4, 4], [S.ACTIVE, S.IDLE, S.FINISHED], [5, 6, 7], [100] * 3, [[1], [2], [3]])
    assert n == [4, 0, 0] and toks[0][:4] == [6, 13, 0, 64]
    _, n, _ = _run_verify(stride, _logits(stride, rows), ids, [0, 4, 4], [S.ACTIVE] * 3, [5, 6, 7], [100, 0, -1], [[1], [2], [3]])
    assert n == [0, 0, 0]


def test_verify_history_is_cut_at_its_row():
    """tokens beyond ld_hist are dropped, the neighbouring row stays as it was"""
    rows = {(0, i): {20 + i: 3.0} for i in range(4)}
    ids = [[1, 20, 21, 22], [2, 0, 0, 0], [3, 0, 0, 0]]
    hist = [list(range(LD_HIST - 2)), [2], [3]]
    _run_verify(4, _logits(4, rows), ids, [4, 1, 1], [S.ACTIVE] * 3, [30, 6, 7], [100] * 3, hist)


# ---- draft ----------------------------------------------------------------------------------------------------------
def _run_draft(stride, k_max, smax, next_ids, state, pos, budget, hist=None, g_max=2, drafts=None):
    ops = _ops()
    i32, i64 = torch.int32, torch.int64
    t = lambda v, dt: torch.tensor(v, dtype=dt).to(DEV)
    ids = torch.full((SLOTS * stride,), -5, dtype=i64, device=DEV)
    blk = torch.full((SLOTS,), -5, dtype=i32, device=DEV)
    kw = {}
    if drafts is not None:
        dt = torch.full((SLOTS, 9), -9, dtype=i64)
        for b, dr in enumerate(drafts):
            dt[b, :len(dr)] = torch.tensor(dr, dtype=i64)
        kw = dict(drafts=dt.to(DEV), n_drafts=t([len(dr) for dr in drafts], i32))
    else:
        h = torch.full((SLOTS, LD_HIST), -1, dtype=i64)
        for b, hh in enumerate(hist):
            h[b, :len(hh)] = torch.tensor(hh, dtype=i64)
        kw = dict(hist=h.to(DEV), hist_len=t([len(hh) for hh in hist], i32), g_max=g_max)
    ops.spec_draft_rows(t(next_ids, i64), t(state, i32), t(pos, i32), t(budget, i32), ids, blk, stride, k_max, smax, pad=PAD, **kw)
    torch.cuda.synchronize()
    got_ids, got_blk = ids.cpu().view(SLOTS, stride).tolist(), blk.cpu().tolist()
    for b in range(SLOTS):
        want = S.draft(next_ids[b], state[b], pos[b], budget[b], stride, k_max, smax, PAD, drafts=None if drafts is None else drafts[b][:9],
                       hist=None if hist is None else hist[b], g_max=g_max)
        assert (got_ids[b], got_blk[b]) == want, (b, got_ids[b], got_blk[b], want)
    return got_ids, got_blk


@pytest.mark.parametrize("stride", [4, 8])
def test_draft_lookup(stride):
    """no match; a match whose continuation runs into the suffix; a history shorter than G (falls to shorter suffixes, or to none)"""
    k = stride - 1
    _, blk = _run_draft(stride, k, 64, [4, 3, 5], [S.ACTIVE] * 3, [9, 9, 9], [100] * 3, [[1, 2, 3, 4], [1, 2, 3, 9, 1, 2, 3], [5, 5]], g_max=3)
    assert blk == [1, min(stride, 5), 2]
    _, blk = _run_draft(stride, k, 64, [5, 3, 3], [S.ACTIVE] * 3, [9, 9, 9], [100] * 3, [[5], [7, 3, 4, 8, 3, 5, 6, 3], [4, 4, 4, 4]], g_max=2)
    assert blk == [1, 4, 2]
    # a history that fills its row, matches at both ends: the most recent earlier occurrence wins
    full = [1, 2, 7] + list(range(30, 30 + LD_HIST - 8)) + [1, 2, 8, 1, 2]
    assert len(full) == LD_HIST
    got, _ = _run_draft(stride, k, 64, [2, 0, 0], [S.ACTIVE, S.IDLE, S.FINISHED], [9, 9, 9], [100] * 3, [full, [1, 1], [1, 1]], g_max=2)
    assert got[0][:2] == [2, 8]


@pytest.mark.parametrize("stride", [4, 8])
def test_draft_caller_form_and_caps(stride):
    """the caller's drafts; the caps by k_max, budget and smax; slots that get no block"""
    k = stride - 1
    d = [[21, 22, 23, 24, 25, 26, 27, 28], [31], []]
    _, blk = _run_draft(stride, k, 64, [4, 3, 5], [S.ACTIVE] * 3, [9, 9, 9], [100] * 3, drafts=d)
    assert blk == [stride, 2, 1]
    _, blk = _run_draft(stride, 2, 64, [4, 3, 5], [S.ACTIVE] * 3, [9, 61, 63], [2, 100, 100], drafts=[d[0]] * 3)
    assert blk == [2, 3, 1]
    _, blk = _run_draft(stride, k, 64, [4, 3, 5], [S.ACTIVE, S.ACTIVE, S.FINISHED], [64, -1, 9], [100, 100, 100], drafts=[d[0]] * 3)
    assert blk == [0, 0, 0]
    _, blk = _run_draft(stride, k, 64, [4, 3, 5], [S.ACTIVE, S.IDLE, S.ACTIVE], [9, 9, 9], [0, 100, 1], drafts=[d[0]] * 3)
    assert blk == [0, 0, 1]


def test_refusals_before_any_launch():
    from llark_amd import _lib
    L = _lib.lib()
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, s = z.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert L.llark_spec_verify_rows(p, LDL, VOCAB, 3, 9, p, p, p, p, p, -1, 0, p, p, p, None, None, 0, s) == -1           # stride
    assert L.llark_spec_verify_rows(p, 96, VOCAB, 3, 4, p, p, p, p, p, -1, 0, p, p, p, None, None, 0, s) == -1            # ldl < vocab
    assert L.llark_spec_verify_rows(p, LDL, VOCAB, 3, 4, p, p, p, p, p, -1, 0, p, p, p, p, None, 8, s) == -1              # hist alone
    assert L.llark_spec_draft_rows(p, p, p, p, None, None, 0, 3, 4, 3, 2, 64, None, None, 0, p, p, 0, s) == -1            # no source
    assert L.llark_spec_draft_rows(p, p, p, p, p, p, 8, 3, 4, 8, 2, 64, None, None, 0, p, p, 0, s) == -1                  # k_max
    assert L.llark_spec_draft_rows(p, p, p, p, p, p, 8, 3, 4, 3, 0, 64, None, None, 0, p, p, 0, s) == -1                  # g_max
    torch.cuda.synchronize()
