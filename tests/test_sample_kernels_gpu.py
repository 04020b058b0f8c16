"""GPU: llark_sample_rows / llark_seen_mark_rows (csrc/sample.hip) against the numpy reference of tests/sample_ref.py.

Steps 1-3 (penalty, temperature, top-k) are fp32 with one rounding each and must be reproduced exactly; the softmax sums are fp32 in
the kernel and float64 in the reference, so the top-p boundary and the draw are held to tol = C_TOL * 2^-24 * Z, with C_TOL = 96
derived in tests/sample_ref.py from the depth of the kernel's sums and the accuracy of expf.  A token whose mass-above lies within
tol of p * Z may fall on either side (the threshold must lie in that band and `kept` must be the count of logits >= it); a draw
whose u * Z lies within tol of a boundary of the cumulative mass may take either neighbour, but at most 1/8 of a case's rows may be
ambiguous in that way (tests/test_sample_ref_cpu.py shows the reference alone stays inside that cap on these inputs)."""
import functools

import numpy as np
import pytest
import torch

import sample_ref as R
from kernel_util import assert_untouched

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
PAD = 5                                  # ldl - vocab; the pad columns hold 1e9: a kernel that read them would pick them
SENT = -7


@functools.lru_cache(maxsize=None)
def _case(vocab, rows):
    return R.make_case(vocab, rows)


@functools.lru_cache(maxsize=None)
def _ref(vocab, rows, name):
    logits, seen, _ = _case(vocab, rows)
    return [R.process(logits[r], seen[r], **R.PARAM_SETS[name]) for r in range(rows)]


def _launch(logits, seen_bool, u, params, slot_of_row=None, state=None, n_slots=None, do_sample=True, **extra):
    """Runs ops.sample_rows on numpy inputs; returns the outputs and the state after the launch as numpy arrays."""
    from llark_amd import ops
    rows, vocab = logits.shape
    n_slots = rows if n_slots is None else n_slots
    buf = torch.full((rows, vocab + PAD), 1e9, dtype=F32)
    buf[:, :vocab] = torch.from_numpy(logits)
    sor = np.arange(rows) if slot_of_row is None else np.asarray(slot_of_row)
    seen = np.zeros((n_slots, (vocab + 31) // 32 + 1), dtype=np.int32)                  # one spare word per row: ld_seen > needed
    seen[sor, :-1] = R.pack_seen(seen_bool)
    seen[:, -1] = 0x5A5A5A5A
    dev = dict(device="cuda")
    t = dict(logits=buf.cuda(), seen=torch.from_numpy(seen).cuda(), choice=torch.full((rows,), SENT, dtype=I64, **dev),
             kept=torch.full((rows,), SENT, dtype=I32, **dev), thresh=torch.full((rows,), float("nan"), dtype=F32, **dev),
             draws=torch.full((n_slots,), 11, dtype=I32, **dev), fallbacks=torch.zeros((1,), dtype=I32, **dev))
    ops.sample_rows(t["logits"], t["choice"], vocab=vocab, state=None if state is None else torch.tensor(state, dtype=I32, **dev),
                    slot_of_row=None if slot_of_row is None else torch.tensor(sor, dtype=I32, **dev), seen=t["seen"], do_sample=do_sample,
                    temperature=params.get("temperature", 1.0), top_k=params.get("top_k", 0), top_p=params.get("top_p", 1.0),
                    repetition_penalty=params.get("theta", 1.0), u=None if u is None else torch.from_numpy(np.asarray(u, dtype=np.float32)).cuda(),
                    draws=t["draws"], kept=t["kept"], thresh=t["thresh"], fallbacks=t["fallbacks"], slots=n_slots, **extra)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["seen_before"] = seen
    assert np.array_equal(out["logits"], buf.numpy(), equal_nan=True)
    return out


def _check_rows(name, out, logits, seen_bool, u, refs, params, active, sor):
    """The four checks of the module docstring on the active rows; everything else must be as it was."""
    rows, vocab = logits.shape
    p = float(np.float32(params.get("top_p", 1.0)))
    ambiguous, worst_band, worst_draw = 0, 0.0, 0.0
    seen_want = out["seen_before"].copy()
    draws_want = np.full(out["draws"].shape, 11, dtype=np.int32)
    for r in range(rows):
        if not active[r]:
            assert out["choice"][r] == SENT and out["kept"][r] == SENT and np.isnan(out["thresh"][r]), f"{name}: skipped row {r} was written"
            continue
        ref, tok, th, kept = refs[r], int(out["choice"][r]), out["thresh"][r], int(out["kept"][r])
        assert 0 <= tok < vocab, f"{name}: row {r} token {tok} outside the vocabulary"
        l, e, in_k = ref["l"], ref["e"], ref["in_k"]
        if p == 1.0:                                                                # exact: the top-k set
            assert th.view(np.int32) == ref["thresh"].view(np.int32) and kept == ref["kept"], (name, r, th, ref["thresh"], kept, ref["kept"])
        else:                                                                       # band around p * Z
            tol = R.tol_of(ref["Z"])
            at = in_k & (l == th)
            assert at.any(), f"{name}: row {r} threshold {th} is no logit of the top-k set"
            assert kept == int((in_k & (l >= th)).sum()), (name, r, kept)
            over = ref["above"][at][0] - p * ref["Z"]                               # kept although mass-above >= p Z by this much
            below = in_k & (l < th)
            under = (p * ref["Z"] - ref["above"][below].min()) if below.any() else 0.0       # dropped although short of p Z by this much
            worst_band = max(worst_band, over / tol, under / tol)
            assert over < tol and under <= tol, (name, r, over / tol, under / tol)
        keep = in_k & (l >= th)
        assert keep[tok], f"{name}: row {r} drew token {tok} outside its kept set"
        want, ok, zk, tol = R.draw(l, e, keep, float(u[r]))
        cum = np.cumsum(np.where(keep, e, 0.0))
        target = float(u[r]) * zk
        worst_draw = max(worst_draw, max((cum[tok - 1] if tok else 0.0) - target, target - cum[tok], 0.0) / tol)
        assert tok in ok, (name, r, tok, want, ok)
        ambiguous += ok.size > 1
        if ok.size == 1:
            assert tok == want
        seen_want.view(np.uint32)[sor[r], tok >> 5] |= np.uint32(1 << (tok & 31))
        draws_want[sor[r]] += 1
    n_act = int(np.sum(active))
    print(f"[ratio] {name}: top-p boundary {worst_band:.3g} of tol, draw {worst_draw:.3g} of tol (tol = {R.C_TOL:g} x 2^-24 Z); "
          f"{ambiguous} of {n_act} rows ambiguous")
    assert ambiguous <= n_act / 8, f"{name}: {ambiguous} of {n_act} rows ambiguous"
    assert_untouched(name + " seen", torch.from_numpy(out["seen"]), torch.from_numpy(seen_want), torch.zeros(seen_want.shape, dtype=torch.bool))
    assert np.array_equal(out["draws"], draws_want) and out["fallbacks"][0] == 0, (name, out["draws"], out["fallbacks"])


SHAPES = [(v, r) for v in R.VOCABS for r in (1, 3, 64)] + [(51203, 3), (65536, 3)]


@pytest.mark.parametrize("name", list(R.PARAM_SETS))
@pytest.mark.parametrize("vocab,rows", SHAPES)
def test_sample_rows_matches_reference(vocab, rows, name):
    """Permuted slot_of_row into a slot table with two spare slots; from 3 rows on, row 1 sits in an IDLE slot and row 2 in a FINISHED
    one and must stay untouched.  51203 and 65536 take the kernel's widest instantiation (3 rows: the shapes are the point)."""
    from llark_amd import ops
    params = R.PARAM_SETS[name]
    logits, seen, u = _case(vocab, rows)
    n_slots = rows + 2
    sor = np.random.default_rng(rows).permutation(n_slots)[:rows]
    state = np.full(n_slots, ops.ROW_ACTIVE, dtype=np.int32)
    state[[b for b in range(n_slots) if b not in sor]] = ops.ROW_IDLE
    active = np.ones(rows, dtype=bool)
    if rows >= 3:
        state[sor[1]], state[sor[2]] = ops.ROW_IDLE, ops.ROW_FINISHED
        active[1:3] = False
    out = _launch(logits, seen, u, params, slot_of_row=sor, state=state, n_slots=n_slots)
    _check_rows(f"sample_rows V{vocab} R{rows} {name}", out, logits, seen, u, _ref(vocab, rows, name), params, active, sor)


EDGE_VOCABS = [1025, 40000]              # the register-only and the LDS-backed instantiation


def _edge_row(vocab, values):
    """A row of -30 .. -20 noise with `values` {token: logit} on top."""
    row = np.random.default_rng(vocab).uniform(-30.0, -20.0, size=vocab).astype(np.float32)
    for t, v in values.items():
        row[t] = v
    return row


@pytest.mark.parametrize("vocab", EDGE_VOCABS)
def test_edge_rows(vocab):
    none = np.zeros((1, vocab), dtype=bool)
    last = vocab - 1
    # k >= vocab keeps everything
    row = _edge_row(vocab, {7: 3.0, last: 2.5})[None]
    out = _launch(row, none, [0.3], dict(top_k=vocab + 10))
    assert out["kept"][0] == vocab and out["thresh"][0] == row.min() and 0 <= out["choice"][0] < vocab and out["fallbacks"][0] == 0
    # k = 1 is greedy whatever T and u
    us = np.array([0.0, 0.5, 1.0 - 2.0 ** -24], dtype=np.float32)
    out = _launch(np.repeat(row, 3, 0), np.repeat(none, 3, 0), us, dict(top_k=1, temperature=0.3))
    assert out["choice"].tolist() == [7, 7, 7] and out["kept"].tolist() == [1, 1, 1] and out["fallbacks"][0] == 0
    # the penalty divides a positive logit and multiplies a negative one: 4 / 2 = 2 < 3, so token 9 wins; -1 * 2 = -2 < -1.5
    row = _edge_row(vocab, {5: 4.0, 9: 3.0})[None]
    seen = none.copy()
    seen[0, 5] = True
    out = _launch(row, seen, None, dict(theta=2.0), do_sample=False)
    assert out["choice"][0] == 9
    row = _edge_row(vocab, {5: -1.0, last: -1.5})[None]
    out = _launch(row, seen, None, dict(theta=2.0), do_sample=False)
    assert out["choice"][0] == last
    out = _launch(row, seen, [0.5], dict(theta=2.0, top_k=2))
    assert out["thresh"][0] == np.float32(-2.0) and out["kept"][0] == 2
    # exact ties at the top-k threshold are all kept
    row = _edge_row(vocab, {3: 5.0, 64: 4.0, 700: 4.0, last: 4.0, 11: 3.0})[None]
    out = _launch(row, none, [0.999], dict(top_k=2))
    assert out["kept"][0] == 4 and out["thresh"][0] == 4.0 and out["choice"][0] in (3, 64, 700, last) and out["fallbacks"][0] == 0
    # -0.0 and +0.0 are one value
    row = _edge_row(vocab, {3: 0.0, 64: -0.0, 11: -1.0})[None]
    out = _launch(row, none, [0.7], dict(top_k=1))
    assert out["kept"][0] == 2 and out["choice"][0] == 64
    # a -inf column is never drawn
    row = np.full((8, vocab), -np.inf, dtype=np.float32)
    row[:, 17], row[:, last] = 1.0, 1.5
    us = (np.arange(8, dtype=np.float32) + 0.5) / 8
    out = _launch(row, np.repeat(none, 8, 0), us, dict(temperature=1.5))
    assert set(out["choice"].tolist()) == {17, last} and out["kept"].tolist() == [vocab] * 8 and out["fallbacks"][0] == 0
    out = _launch(row, np.repeat(none, 8, 0), us, dict(top_p=0.99))
    assert set(out["choice"].tolist()) == {17, last} and out["kept"].tolist() == [2] * 8 and out["fallbacks"][0] == 0
    # degenerate rows: in-range greedy token, counted
    bad = np.stack([_edge_row(vocab, {40: np.nan, 90: np.nan, 3: 50.0}), np.full(vocab, -np.inf, dtype=np.float32),
                    _edge_row(vocab, {last: np.inf, 3: 50.0}), _edge_row(vocab, {3: 1.0})])
    out = _launch(bad, np.repeat(none, 4, 0), [0.5] * 4, dict(temperature=0.8, top_k=50, top_p=0.9))
    assert out["choice"].tolist() == [40, 0, last, 3] and out["fallbacks"][0] == 3 and out["kept"].tolist()[:3] == [0, 0, 0]
    assert out["draws"].tolist() == [12] * 4


@pytest.mark.parametrize("vocab", [63, 1025, 32003, 50435])
def test_greedy_mode_is_argmax_of_the_penalised_row(vocab):
    rows = 5
    logits, seen, _ = _case(vocab, 64)
    logits, seen = logits[:rows], seen[:rows]
    out = _launch(logits, seen, None, dict(theta=1.3), do_sample=False)
    pen = np.stack([R.penalise(logits[r], seen[r], 1.3) for r in range(rows)])
    want = torch.argmax(torch.from_numpy(pen), dim=-1).numpy()
    assert np.array_equal(out["choice"], want)
    assert out["draws"].tolist() == [11] * rows and out["kept"].tolist() == [SENT] * rows and out["fallbacks"][0] == 0
    for r in range(rows):                                      # the chosen token is now seen; nothing else changed
        t = int(want[r])
        w = out["seen"][r].view(np.uint32).copy()
        assert (w[t >> 5] >> (t & 31)) & 1
        w[t >> 5] &= ~np.uint32(1 << (t & 31)) | out["seen_before"][r].view(np.uint32)[t >> 5]
        assert np.array_equal(w, out["seen_before"][r].view(np.uint32))


def test_refused_arguments_return_their_status_and_launch_nothing():
    from llark_amd import _lib, ops
    L = _lib.lib()
    V, rows = 100, 2
    lg = torch.zeros((rows, V), device="cuda")
    ch = torch.full((rows,), SENT, dtype=I64, device="cuda")
    seen = torch.zeros((rows, 4), dtype=I32, device="cuda")
    dr = torch.zeros((rows,), dtype=I32, device="cuda")
    u = torch.zeros((rows,), device="cuda")
    s = ops._stream()
    N = None

    def call(logits=lg.data_ptr(), ldl=V, vocab=V, rows_=rows, slots=rows, seen_=seen.data_ptr(), ld_seen=4, do_sample=1, T=1.0, k=0, p=1.0,
             theta=1.0, u_=u.data_ptr(), draws=dr.data_ptr(), choice=ch.data_ptr()):
        return L.llark_sample_rows(logits, ldl, vocab, rows_, slots, N, N, seen_, ld_seen, do_sample, T, k, p, theta, u_, 0, draws, N, choice, N, N,
                                   N, s)
    INV, UNS = -1, -2
    for want, kw in [(INV, dict(logits=N)), (INV, dict(choice=N)), (INV, dict(ldl=V - 1)), (INV, dict(vocab=0)), (INV, dict(rows_=0)),
                     (INV, dict(rows_=3)), (INV, dict(T=0.0)), (INV, dict(T=-1.0)), (INV, dict(p=0.0)), (INV, dict(p=1.5)), (INV, dict(theta=0.0)),
                     (INV, dict(theta=-2.0)), (INV, dict(seen_=N, theta=1.3)), (INV, dict(ld_seen=3)), (INV, dict(u_=N, draws=N)), (INV, dict(k=-1)),
                     (UNS, dict(vocab=65537, ldl=65537, seen_=N))]:
        assert call(**kw) == want, kw
        assert L.llark_last_error().startswith(b"sample_rows:")
    assert call(do_sample=0, T=0.0, p=0.0, u_=N, draws=N) == 0                      # greedy mode does not look at the sampling scalars
    torch.cuda.synchronize()
    assert ch.tolist() == [0, 0] and dr.tolist() == [0, 0]                          # only the accepted call launched
    ids = torch.zeros((4,), dtype=I64, device="cuda")
    of = torch.zeros((1,), dtype=I32, device="cuda")
    assert L.llark_seen_mark_rows(N, 4, of.data_ptr(), of.data_ptr(), N, 1, rows, V, seen.data_ptr(), 4, s) == INV
    assert L.llark_seen_mark_rows(ids.data_ptr(), 4, of.data_ptr(), of.data_ptr(), N, 1, rows, V, seen.data_ptr(), 3, s) == INV
    assert L.llark_seen_mark_rows(ids.data_ptr(), 4, of.data_ptr(), of.data_ptr(), N, 3, rows, V, seen.data_ptr(), 4, s) == INV


def test_seen_mark_rows_sets_exactly_the_listed_bits():
    from llark_amd import ops
    V, slots = 1000, 4
    g = np.random.default_rng(5)
    lists = [g.integers(-5, V + 5, size=n) for n in (0, 1, 300, 77)]            # ids outside [0, V) are ignored
    offs = np.cumsum([0] + [len(x) for x in lists[:-1]]).astype(np.int32)
    sor = np.array([2, 0, 3, 1], dtype=np.int32)
    seen = torch.full((slots, 33), 0, dtype=I32)
    seen[:, 32] = 0x1234
    seen[3, 0] = 1 << 9                                                             # bits already there stay
    want = seen.numpy().copy().view(np.uint32)
    for r, ids in enumerate(lists):
        for t in ids:
            if 0 <= t < V:
                want[sor[r], t >> 5] |= np.uint32(1 << (t & 31))
    dev = seen.cuda()
    ops.seen_mark_rows(torch.from_numpy(np.concatenate(lists).astype(np.int64)).cuda(), torch.from_numpy(offs).cuda(),
                       torch.tensor([len(x) for x in lists], dtype=I32).cuda(), dev, V, slot_of_row=torch.from_numpy(sor).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), want)


def test_philox_draws_equal_the_reference_stream_over_two_launches():
    """u == NULL: the tokens are those of a run that is handed the reference's Philox u for (seed, stream id, draw number); two
    launches in a row cover the counter advance, stream ids above 2^32 the high counter words, the seed both key words."""
    from llark_amd import ops
    vocab, rows = 1025, 8
    logits, seen, _ = _case(vocab, 64)
    logits, seen = logits[:rows], seen[:rows]
    seed = (5 << 32) | 9
    sids = [0, 1, 2, (1 << 32) + 1, (1 << 40) + 3, (1 << 62) + 5, 77, 4095]
    params = dict(temperature=1.3)                                                   # flat enough that tokens vary with u
    lg = torch.from_numpy(logits).cuda()
    sn = torch.from_numpy(R.pack_seen(seen)).cuda()
    draws = torch.zeros((rows,), dtype=I32, device="cuda")
    sid = torch.tensor(sids, dtype=I64, device="cuda")
    got = []
    for _ in range(2):
        ch = torch.full((rows,), SENT, dtype=I64, device="cuda")
        ops.sample_rows(lg, ch, seen=sn, draws=draws, stream_id=sid, seed=seed, **params)
        got.append(ch.cpu().numpy())
    assert draws.tolist() == [2] * rows
    for n in range(2):
        u = np.array([R.philox_uniform(seed, s, n) for s in sids], dtype=np.float32)
        out = _launch(logits, seen, u, params)
        assert np.array_equal(got[n], out["choice"]), (n, got[n], out["choice"])
    assert (got[0] != got[1]).any()


def test_distribution_of_4096_streams():
    """4096 rows share one 16-token row of known probabilities, stream ids 0 .. 4095, one launch: every token's count lies within
    5 sigma of 4096 p (deterministic for this seed)."""
    from llark_amd import ops
    n = 4096
    probs = np.array([20, 16, 12, 10, 8, 7, 6, 5, 4, 3, 3, 2, 1.5, 1, 1, 0.5], dtype=np.float64)
    probs /= probs.sum()
    lg = torch.from_numpy(np.log(probs).astype(np.float32)).repeat(n, 1).cuda()
    p32 = np.exp(np.log(probs).astype(np.float32).astype(np.float64))
    p32 /= p32.sum()
    ch = torch.full((n,), SENT, dtype=I64, device="cuda")
    draws = torch.zeros((n,), dtype=I32, device="cuda")
    ops.sample_rows(lg, ch, draws=draws, stream_id=torch.arange(n, dtype=I64, device="cuda"), seed=20240229)
    counts = np.bincount(ch.cpu().numpy(), minlength=16)
    assert counts.sum() == n and counts.size == 16
    sigma = np.sqrt(n * p32 * (1 - p32))
    z = (counts - n * p32) / sigma
    print("[ratio] distribution: worst |count - n p| / sigma = %.2f" % np.abs(z).max())
    assert (np.abs(z) <= 5).all(), z
