"""GPU: llark_token_logprob_rows (csrc/logprob.hip) against the float64 reference of tests/logprob_ref.py.

``rank`` is an integer count and must be exact.  ``logprob`` is held to tol = 2^-24 (2 |l_t - M| + |lp| + D + E + 4) of the float64
value: the two subtractions and logf (first two terms), D = ceil(vocab / 1024) + 21 additions on the longest path of the kernel's sum
(per thread in column order, 6 butterfly steps over the lanes, 15 additions of the 16 wave sums; 71 at vocab 50 435), the rounding of
the exponent arguments weighted by the row's own distribution (E, from the reference), expf and slack (4).  Rows that are skipped
(idle / finished / out-of-range slot, token -1 or vocab) must leave every output and every history entry bit-identical."""
import functools

import numpy as np
import pytest
import torch

import logprob_ref as R
from kernel_util import bits

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
SENT_LP, SENT_RK, SENT_H = -1234.5, -7, 77.25
WIDTH = 3                                 # ld_hist of the sentinel history; every slot starts at count 1, total 0.5

# 4096 | 4097, 32768 | 32769 and 51200 | 51201 are the edges between the kernel's instantiations; from 51 201 on the columns beyond
# 51 200 are read in a loop (52 303: two trips for some threads, one for others)
VOCABS = (1, 63, 257, 1025, 32003, 50435)
SHAPES = [(v, r) for v in VOCABS for r in (1, 3, 64)] + [(v, 3) for v in (4096, 4097, 32768, 32769, 51200, 51201, 52303)]
LAYOUTS = ("tight", "pad_1e9", "pad_nan")


@functools.lru_cache(maxsize=None)
def _case(vocab, rows):
    """(logits, tokens, reference lp / rank / tol per row).  Targets cycle through index 0, vocab - 1, the maximum, a -inf logit and a
    random index."""
    logits = R.make_rows(vocab, rows)
    rng = np.random.default_rng(vocab * 31 + rows)
    tokens = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        kind = r % 5
        if kind == 0:
            tokens[r] = 0
        elif kind == 1:
            tokens[r] = vocab - 1
        elif kind == 2:
            tokens[r] = int(logits[r].argmax())
        elif kind == 3 and vocab > 1:
            tokens[r] = int(rng.integers(0, vocab))
            logits[r, tokens[r]] = -np.inf
            logits[r, (tokens[r] + 1) % vocab] = -np.inf        # and one that is no target: adds 0 to S
        else:
            tokens[r] = int(rng.integers(0, vocab))
    ref = [R.row_logprob(logits[r], int(tokens[r])) for r in range(rows)]
    tols = [R.tol_of(logits[r], int(tokens[r])) for r in range(rows)]
    logits.setflags(write=False)
    return logits, tokens, ref, tols


def _device_logits(logits, layout, front=0):
    """The rows inside a flat buffer, `front` floats in: ldl == vocab ("tight": most rows are not 16-byte aligned) or ldl = vocab rounded
    up to 64 with the pad columns holding 1e9 / NaN, which a kernel that read them would show."""
    rows, vocab = logits.shape
    ldl = vocab if layout == "tight" else (vocab + 63) // 64 * 64 if isinstance(layout, str) else int(layout)
    fill = float("nan") if layout == "pad_nan" else 1e9
    flat = torch.full((front + rows * ldl + 5,), fill, dtype=F32)
    view = flat[front:front + rows * ldl].view(rows, ldl)
    view[:, :vocab] = torch.from_numpy(np.array(logits))
    dev = flat.cuda()
    return dev[front:front + rows * ldl].view(rows, ldl), dev, flat


def _launch(logits, tokens, layout="tight", slot_of_row=None, state=None, n_slots=None, count0=1, width=WIDTH, front=0, with_rank=True):
    from llark_amd import ops
    rows, vocab = logits.shape
    n_slots = rows if n_slots is None else n_slots
    lg, dev_flat, flat = _device_logits(logits, layout, front)
    dev = dict(device="cuda")
    t = dict(logprob=torch.full((rows,), SENT_LP, dtype=F32, **dev), rank=torch.full((rows,), SENT_RK, dtype=I32, **dev),
             hist=torch.full((n_slots, width), SENT_H, dtype=F32, **dev), count=torch.full((n_slots,), count0, dtype=I32, **dev),
             total=torch.full((n_slots,), 0.5, dtype=F32, **dev))
    ops.token_logprob_rows(lg, torch.as_tensor(np.asarray(tokens), dtype=I64).cuda(), t["logprob"], vocab=vocab,
                           rank=t["rank"] if with_rank else None, state=None if state is None else torch.tensor(state, dtype=I32, **dev),
                           slot_of_row=None if slot_of_row is None else torch.tensor(np.asarray(slot_of_row), dtype=I32, **dev),
                           hist=t["hist"], count=t["count"], total=t["total"], slots=n_slots)
    torch.cuda.synchronize()
    assert torch.equal(bits(dev_flat), bits(flat)), "the logits were written"
    return {k: v.cpu().numpy() for k, v in t.items()}


def _check(name, out, logits, tokens, ref, tols, active, sor, count0=1, width=WIDTH):
    rows, vocab = logits.shape
    n_slots = out["count"].shape[0]
    hist_want = np.full((n_slots, width), SENT_H, dtype=np.float32)
    count_want = np.full(n_slots, count0, dtype=np.int32)
    total_want = np.full(n_slots, 0.5, dtype=np.float32)
    worst = 0.0
    for r in range(rows):
        got, rk = out["logprob"][r], int(out["rank"][r])
        if not active[r]:
            assert got == np.float32(SENT_LP) and rk == SENT_RK, f"{name}: skipped row {r} was written"
            continue
        lp, rank, _ = ref[r]
        assert rk == rank, f"{name}: row {r} rank {rk}, reference {rank}"
        if np.isnan(lp):
            assert np.isnan(got), (name, r, got)
        elif np.isinf(lp):
            assert got == lp, (name, r, got, lp)
        else:
            err = abs(float(got) - lp)
            worst = max(worst, err / tols[r])
            assert err <= tols[r], f"{name}: row {r} token {tokens[r]} logprob {got} vs {lp}: {err / tols[r]:.3g} of tol"
        s = sor[r]
        if count_want[s] < width:
            hist_want[s, count_want[s]] = got
        with np.errstate(all="ignore"):
            total_want[s] = np.float32(total_want[s]) + np.float32(got)
        count_want[s] += 1
    print(f"[ratio] {name}: worst logprob error {worst:.3g} of tol (D = {R.depth(vocab)})")
    assert np.array_equal(out["hist"].view(np.int32), hist_want.view(np.int32)), f"{name}: history"
    assert np.array_equal(out["count"], count_want), f"{name}: count {out['count']} vs {count_want}"
    assert np.array_equal(out["total"].view(np.int32), total_want.view(np.int32)), f"{name}: total"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("vocab,rows", SHAPES)
def test_token_logprob_rows_matches_reference(vocab, rows, layout):
    """Permuted slot_of_row into a slot table with two spare slots; from 3 rows on, row 1 sits in an IDLE slot and row 2 in a FINISHED
    one; at 64 rows, rows 5 .. 8 carry the tokens -1 / vocab and the slots -1 / n_slots.  All of those must stay untouched."""
    logits, tokens, ref, tols = _case(vocab, rows)
    tokens = tokens.copy()
    n_slots = rows + 2
    sor = np.random.default_rng(rows).permutation(n_slots)[:rows]
    state = np.full(n_slots, R.ROW_ACTIVE, dtype=np.int32)
    state[[b for b in range(n_slots) if b not in sor]] = R.ROW_IDLE
    active = np.ones(rows, dtype=bool)
    if rows >= 3:
        state[sor[1]], state[sor[2]] = R.ROW_IDLE, R.ROW_FINISHED
        active[1:3] = False
    if rows >= 9:
        tokens[5], tokens[6] = -1, vocab
        sor[7], sor[8] = -1, n_slots
        active[5:9] = False
    out = _launch(logits, tokens, layout, slot_of_row=sor, state=state, n_slots=n_slots)
    _check(f"token_logprob_rows V{vocab} R{rows} {layout}", out, logits, tokens, ref, tols, active, sor)


@pytest.mark.parametrize("vocab", [1025, 40000, 52303])
def test_edge_rows(vocab):
    last = vocab - 1
    rng = np.random.default_rng(vocab)
    # ties: only strictly larger logits count
    row = rng.uniform(-30.0, -20.0, size=vocab).astype(np.float32)
    row[[3, 64, last]] = 5.0
    row[[11, 700]] = 3.0
    rows = np.repeat(row[None], 4, 0)
    toks = np.array([64, last, 700, 12])
    out = _launch(rows, toks)
    assert out["rank"].tolist() == [0, 0, 3, int((row > row[12]).sum())]
    assert bits(torch.from_numpy(out["logprob"][:1])).item() == bits(torch.from_numpy(out["logprob"][1:2])).item()
    # magnitude 3e4: nothing overflows
    big = (1e4 * rng.standard_normal((3, vocab))).astype(np.float32).clip(-3e4, 3e4)
    big[0, 5], big[1, last], big[2, 0] = 3e4, 3e4, -3e4
    toks = np.array([5, 7, 0])
    ref = [R.row_logprob(big[r], int(toks[r])) for r in range(3)]
    tols = [R.tol_of(big[r], int(toks[r])) for r in range(3)]
    out = _launch(big, toks)
    assert np.isfinite(out["logprob"]).all()
    _check(f"3e4 rows V{vocab}", out, big, toks, ref, tols, [True] * 3, [0, 1, 2])
    # degenerate rows: a NaN, a +inf maximum, all -inf -> NaN and rank -1; the history still advances
    bad = np.stack([row.copy(), row.copy(), np.full(vocab, -np.inf, dtype=np.float32), row.copy()])
    bad[0, 40], bad[0, last] = np.nan, np.nan
    bad[1, last] = np.inf
    toks = np.array([3, 3, 0, 3])
    out = _launch(bad, toks)
    assert np.isnan(out["logprob"][:3]).all() and out["rank"].tolist()[:3] == [-1, -1, -1]
    assert np.isfinite(out["logprob"][3]) and out["rank"][3] == 0 and out["count"].tolist() == [2] * 4
    # no rank asked for
    out = _launch(rows, np.array([64, last, 700, 12]), with_rank=False)
    assert out["rank"].tolist() == [SENT_RK] * 4 and np.isfinite(out["logprob"]).all()


def test_full_history_and_two_launches_accumulate():
    from llark_amd import ops
    vocab, rows = 1025, 3
    logits, _, _, _ = _case(vocab, 64)
    logits = logits[8:8 + rows]
    toks = np.array([1, 2, 3])
    ref = [R.row_logprob(logits[r], int(toks[r])) for r in range(rows)]
    tols = [R.tol_of(logits[r], int(toks[r])) for r in range(rows)]
    for count0 in (WIDTH, WIDTH + 4):                       # full: no hist write, count and total still advance
        out = _launch(logits, toks, count0=count0)
        _check(f"full history count0={count0}", out, logits, toks, ref, tols, [True] * rows, [0, 1, 2], count0=count0)
        assert (out["hist"] == SENT_H).all()
    lg = torch.from_numpy(np.array(logits)).cuda()
    hist = torch.full((rows, 2), SENT_H, dtype=F32, device="cuda")
    count = torch.zeros((rows,), dtype=I32, device="cuda")
    total = torch.zeros((rows,), dtype=F32, device="cuda")
    lps = []
    for step in range(3):
        tk = torch.as_tensor(toks + step, dtype=I64).cuda()
        lps.append(ops.token_logprob_rows(lg, tk, torch.empty((rows,), dtype=F32, device="cuda"), hist=hist, count=count, total=total).cpu())
    assert count.tolist() == [3] * rows
    assert torch.equal(bits(hist), bits(torch.stack(lps[:2], 1)))
    assert torch.equal(bits(total), bits((lps[0] + lps[1]) + lps[2]))
    # total alone, count alone
    total.zero_()
    ops.token_logprob_rows(lg, tk, torch.empty((rows,), dtype=F32, device="cuda"), total=total)
    assert torch.equal(bits(total), bits(lps[2]))
    ops.token_logprob_rows(lg, tk, torch.empty((rows,), dtype=F32, device="cuda"), count=count)
    assert count.tolist() == [4] * rows


@pytest.mark.parametrize("vocab", [1025, 50435, 52303])
def test_a_row_gives_the_same_bits_wherever_it_sits(vocab):
    """The same row at another r, slot, row count, ldl and alignment, and the same launch twice: bit-equal logprob and rank."""
    logits, tokens, _, _ = _case(vocab, 3)
    row, t = logits[0], int(tokens[2])
    a = _launch(row[None], [t])
    again = _launch(row[None], [t])
    filler = R.make_rows(vocab, 5, seed=3)
    got = [(a["logprob"][0], a["rank"][0]), (again["logprob"][0], again["rank"][0])]
    for r, ldl, front in ((3, vocab + 3, 1), (0, vocab + 2, 2), (4, (vocab + 63) // 64 * 64, 3), (1, vocab, 0)):
        many = filler.copy()
        many[r] = row
        toks = np.full(5, 1, dtype=np.int64)
        toks[r] = t
        sor = np.array([6, 2, 0, 5, 3])
        out = _launch(many, toks, layout=ldl, slot_of_row=sor, n_slots=7, front=front)
        got.append((out["logprob"][r], out["rank"][r]))
        assert out["hist"][sor[r], 1].view(np.int32) == out["logprob"][r].view(np.int32)
    assert len({(lp.view(np.int32).item(), int(rk)) for lp, rk in got}) == 1, got


def test_refused_arguments_return_their_status_and_launch_nothing():
    from llark_amd import _lib, ops
    L = _lib.lib()
    V, rows = 100, 2
    lg = torch.zeros((rows, V), device="cuda")
    tk = torch.zeros((rows,), dtype=I64, device="cuda")
    lp = torch.full((rows,), SENT_LP, dtype=F32, device="cuda")
    hist = torch.full((rows, 4), SENT_H, dtype=F32, device="cuda")
    cnt = torch.zeros((rows,), dtype=I32, device="cuda")
    s = ops._stream()
    N = None

    def call(logits=lg.data_ptr(), ldl=V, vocab=V, rows_=rows, slots=rows, sor=N, tokens=tk.data_ptr(), logprob=lp.data_ptr(), hist_=N, ld_hist=0,
             count=N):
        return L.llark_token_logprob_rows(logits, ldl, vocab, rows_, slots, N, sor, tokens, logprob, N, hist_, ld_hist, count, N, s)
    INV = -1
    for kw in [dict(logits=N), dict(tokens=N), dict(logprob=N), dict(rows_=0), dict(slots=0), dict(vocab=0), dict(vocab=-3), dict(ldl=V - 1),
               dict(rows_=3), dict(slots=1), dict(hist_=hist.data_ptr(), ld_hist=4), dict(hist_=hist.data_ptr(), ld_hist=0, count=cnt.data_ptr()),
               dict(hist_=hist.data_ptr(), ld_hist=-1, count=cnt.data_ptr())]:
        assert call(**kw) == INV, kw
        assert L.llark_last_error().startswith(b"token_logprob_rows:")
    torch.cuda.synchronize()
    assert lp.tolist() == [SENT_LP] * rows and cnt.tolist() == [0, 0] and (hist == SENT_H).all()     # nothing launched
    assert call(hist_=hist.data_ptr(), ld_hist=4, count=cnt.data_ptr()) == 0
    torch.cuda.synchronize()
    want = np.float32(-np.log(np.float64(V)))
    assert abs(lp[0].item() - want) <= 2.0 ** -24 * (abs(want) + R.depth(V) + 4) and cnt.tolist() == [1, 1]


def test_a_cpu_tensor_raises():
    from llark_amd import _lib, ops
    with pytest.raises(_lib.LlarkHipError):
        ops.token_logprob_rows(torch.zeros((2, 8)), torch.zeros((2,), dtype=I64), torch.zeros((2,)))
    with pytest.raises(_lib.LlarkHipError):
        ops.token_logprob_rows(torch.zeros((2, 8), device="cuda"), torch.zeros((2,), dtype=I64), torch.zeros((2,), device="cuda"))
