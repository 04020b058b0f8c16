"""GPU: the three kernels of the beam step (csrc/beam.hip) against the float64 reference of tests/beam_ref.py.

llark_beam_topk_rows: the candidates' log-probabilities must have the bits of llark_token_logprob_rows; a score is held to beam_ref.cand_tols
(logprob_ref.tol_of for the log-probability plus half an ulp of the sum); the (token) order must be the reference's wherever adjacent
reference candidates differ by more than their two tolerances -- the rows are built (beam_ref.make_rows) and their seeds chosen so that no
such near tie exists, and the count is asserted to be 0.  llark_beam_advance is a merge of fp32 values: fed the device's own candidates,
the reference must reproduce every integer and every fp32 of the state exactly (a hypothesis score, one double-precision pow away, to one
ulp).  llark_kv_copy_slots moves bits."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
from kernel_util import bits
from llark_amd import _lib, ops
from llark_amd.m2t.beam import BeamSearch

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
SENT_S, SENT_T, SENT_L = -4321.5, -9, 55.25
ROWS = 64
# seeds of beam_ref.make_rows per (vocab, beams), chosen on the CPU with beam_ref.near_ties alone so that no case has a near tie: seed 0
# qualifies for every case below, so none is listed
SEEDS = {}


def _seed(vocab, beams):
    return SEEDS.get((vocab, beams), 0)


@functools.lru_cache(maxsize=None)
def _case(vocab, beams):
    """64 rows, their slots' scores in [-20, 0), the reference's 2B + 1 best candidates of every row and the tolerances."""
    logits = R.make_rows(vocab, ROWS, _seed(vocab, beams))
    rng = np.random.default_rng(vocab + 97 * beams)
    score = rng.uniform(-20.0, 0.0, ROWS).astype(np.float32)
    ref = [R.row_candidates(logits[r], score[r], beams, 2 * beams + 1) for r in range(ROWS)]
    tols = [R.cand_tols(logits[r], score[r], ref[r][1], ref[r][0]) for r in range(ROWS)]
    near = sum(R.near_ties(logits[r], score[r], beams) for r in range(ROWS))
    logits.setflags(write=False)
    return logits, score, ref, tols, near


def _padded(logits, fill=1e9):
    """ldl = vocab rounded up to 64, + 64: the pad columns hold a value that a kernel which read them would show."""
    rows, vocab = logits.shape
    ldl = (vocab + 63) // 64 * 64 + 64
    buf = torch.full((rows, ldl), fill, dtype=F32)
    buf[:, :vocab] = torch.from_numpy(np.ascontiguousarray(logits))
    return buf.cuda()


def _outs(rows, K):
    return (torch.full((rows, K), SENT_S, dtype=F32, device="cuda"), torch.full((rows, K), SENT_T, dtype=I32, device="cuda"),
            torch.full((rows, K), SENT_L, dtype=F32, device="cuda"))


@pytest.mark.parametrize("beams", [1, 3, 16])
@pytest.mark.parametrize("vocab", [32, 1000, 32003, 50435, 51201])
def test_topk_rows_values_order_bits_and_skips(vocab, beams):
    logits, score, ref, tols, near = _case(vocab, beams)
    K = 2 * beams
    dev = _padded(logits)
    # 64 rows on 70 slots, in a shuffled slot order; slots 3 (idle), 11 (finished) and rows 5 (slot -1), 6 (slot 70) are skipped
    perm = np.random.default_rng(5).permutation(70)[:ROWS].astype(np.int32)
    perm[5], perm[6] = -1, 70
    state = torch.full((70,), ops.ROW_ACTIVE, dtype=I32)
    state[3], state[11] = ops.ROW_IDLE, ops.ROW_FINISHED
    skipped = [r for r in range(ROWS) if not 0 <= perm[r] < 70 or int(state[perm[r]]) != ops.ROW_ACTIVE]
    assert len(skipped) >= 2
    sc = torch.zeros((70,), dtype=F32)
    for r in range(ROWS):
        if 0 <= perm[r] < 70:
            sc[perm[r]] = float(score[r])
    cs, ct, cl = _outs(ROWS, K)
    fb = torch.zeros((1,), dtype=I32, device="cuda")
    ops.beam_topk_rows(dev, sc.cuda(), beams, cs, ct, cl, vocab=vocab, state=state.cuda(), slot_of_row=torch.from_numpy(perm).cuda(), fallbacks=fb)
    hs, ht, hl = cs.cpu().numpy(), ct.cpu().numpy(), cl.cpu().numpy()
    assert int(fb.item()) == 0
    for r in skipped:
        assert (hs[r] == np.float32(SENT_S)).all() and (ht[r] == SENT_T).all() and (hl[r] == np.float32(SENT_L)).all(), f"row {r} was written"
    print(f"vocab {vocab} beams {beams}: {near} near ties among the reference's candidates")
    assert near == 0
    worst = 0.0
    for r in range(ROWS):
        if r in skipped:
            continue
        c, t, lp = ref[r]
        assert ht[r].tolist() == t[:K].tolist(), f"row {r}: tokens {ht[r].tolist()} vs {t[:K].tolist()}"
        err = np.abs(hs[r].astype(np.float64) - c[:K])
        worst = max(worst, float((err / tols[r][:K]).max()))
        assert (err <= tols[r][:K]).all(), f"row {r}: scores off by {err / tols[r][:K]} of tol"
        # the score is the one fp32 addition of the slot's score and the log-probability that was stored
        assert (hs[r] == (score[r] + hl[r]).astype(np.float32)).all()
    print(f"worst score error {worst:.3g} of tol")
    # log-probabilities: the bits of llark_token_logprob_rows for the same row and token
    for k in range(K):
        toks = ct[:, k].to(I64).contiguous()
        toks[torch.tensor(skipped, device="cuda")] = -1
        want = ops.token_logprob_rows(dev, toks, torch.full((ROWS,), SENT_L, dtype=F32, device="cuda"), vocab=vocab)
        assert torch.equal(bits(want), bits(cl[:, k].contiguous())), f"candidate {k}: log-probabilities differ from token_logprob_rows"
    # a row gives the same bits wherever it sits: alone, and among B rows, in a tight layout at another alignment
    for rows in (1, beams):
        pick = [r for r in range(ROWS) if r not in skipped][7:7 + rows]
        tight = torch.empty((rows * vocab + 3,), dtype=F32, device="cuda")[3:].view(rows, vocab)
        tight.copy_(dev[pick, :vocab])
        s2 = torch.from_numpy(score[pick]).cuda()
        a, b, c2 = _outs(rows, K)
        ops.beam_topk_rows(tight, s2, beams, a, b, c2)
        for got, full in ((a, cs), (b, ct), (c2, cl)):
            assert torch.equal(bits(got), bits(full[pick].contiguous()))


def test_topk_rows_exact_ties_follow_the_rule():
    """Equal logits in one row: token ascending.  Identical rows with equal scores: identical candidates."""
    V, B = 1000, 3
    row = np.zeros((4, V), dtype=np.float32)
    row[1, [900, 17, 400]] = 2.0                               # three tied leaders, then everything else tied
    row[2] = row[1]
    row[3, ::2] = 1.0
    cs, ct, cl = _outs(4, 2 * B)
    ops.beam_topk_rows(torch.from_numpy(row).cuda(), torch.tensor([0.0, -1.5, -1.5, -1e9]).cuda(), B, cs, ct, cl)
    t = ct.cpu().tolist()
    assert t[0] == [0, 1, 2, 3, 4, 5] and t[1] == [17, 400, 900, 0, 1, 2] and t[3] == [0, 1, 2, 3, 4, 5]
    for x in (cs, ct, cl):
        assert torch.equal(bits(x[1].contiguous()), bits(x[2].contiguous()))
    c = cs.cpu()
    assert (c[:, :-1] >= c[:, 1:]).all() and float(c[3, 0]) == -1e9      # at -1e9 every candidate rounds to the score: all tied


def test_topk_rows_without_a_distribution():
    V, B = 5000, 2
    x = torch.from_numpy(R.make_rows(V, 5, 3).copy())
    x[0, 4999] = float("nan")
    x[1, 17] = float("inf")
    x[2] = float("-inf")
    x[3, 100:4000] = float("-inf")                             # a proper row with -inf logits: they add 0 and come last
    cs, ct, cl = _outs(5, 2 * B)
    fb = torch.zeros((1,), dtype=I32, device="cuda")
    ops.beam_topk_rows(x.cuda(), torch.zeros(5).cuda(), B, cs, ct, cl, fallbacks=fb)
    assert int(fb.item()) == 3
    for r in range(3):
        assert ct[r].tolist() == [-1] * 4 and torch.isinf(cs[r]).all() and (cs[r] < 0).all() and torch.isinf(cl[r]).all()
    for r in (3, 4):
        c, t, lp = R.row_candidates(x[r].numpy(), 0.0, B)
        assert ct[r].tolist() == t.tolist() and np.allclose(cs[r].cpu().numpy(), c, atol=1e-4)
    x2 = torch.full((1, 64), float("-inf"))
    x2[0, [5, 9]] = torch.tensor([1.0, 0.0])                   # fewer finite logits than 2B: the rest are -inf candidates, lowest tokens first
    cs, ct, cl = _outs(1, 4)
    ops.beam_topk_rows(x2.cuda(), torch.zeros(1).cuda(), 2, cs, ct, cl)
    assert ct[0].tolist() == [5, 9, 0, 1] and torch.isinf(cs[0, 2:]).all() and torch.isfinite(cs[0, :2]).all()


def _rc(fn, *args):
    rc = fn(*args)
    return rc, _lib.lib().llark_last_error().decode()


def test_refused_arguments_return_invalid_and_launch_nothing():
    L = _lib.lib()
    V, B = 100, 2
    lg = torch.zeros((2, V), dtype=F32, device="cuda")
    sc = torch.zeros((2,), dtype=F32, device="cuda")
    cs, ct, cl = _outs(2, 2 * B)
    p = lambda t: t.data_ptr()                                                 # noqa: E731
    topk = lambda **kw: {**dict(logits=p(lg), ldl=V, vocab=V, rows=2, slots=2, score=p(sc), beams=B, cs=p(cs)), **kw}   # noqa: E731
    for kw, word in ((dict(logits=None), "null"), (dict(score=None), "null"), (dict(cs=None), "null"), (dict(beams=0), "beams"),
                     (dict(beams=17), "beams"), (dict(vocab=3), "vocab"), (dict(ldl=V - 1), "ldl"), (dict(rows=0), "rows"),
                     (dict(rows=3), "rows")):
        a = topk(**kw)
        rc, msg = _rc(L.llark_beam_topk_rows, a["logits"], a["ldl"], a["vocab"], a["rows"], a["slots"], None, None, a["score"], a["beams"],
                      a["cs"], p(ct), p(cl), None, None)
        assert rc == -1 and "beam_topk_rows" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (cs == SENT_S).all() and (ct == SENT_T).all() and (cl == SENT_L).all()

    bs = BeamSearch(1, B, V, 4, "cuda")
    st = torch.full((B,), ops.ROW_ACTIVE, dtype=I32, device="cuda")
    before = [t.clone() for t in (bs.score, bs.rank_of_slot, bs.heap, bs.heap_meta, bs.done, bs.trellis, bs.pairs, bs.cur_len, st)]

    def advance(**kw):
        a = {**dict(cs=p(bs.cand_score), n=1, beams=B, step=0, max_steps=4, lp=1.0, score=p(bs.score), trellis=p(bs.trellis)), **kw}
        return _rc(L.llark_beam_advance, a["cs"], p(bs.cand_token), p(bs.cand_logprob), a["n"], a["beams"], a["step"], a["max_steps"], -1, 0,
                   a["lp"], 0, a["score"], p(bs.rank_of_slot), p(st), None, p(bs.cur_len), p(bs.next_ids), p(bs.heap), p(bs.heap_meta),
                   p(bs.done), a["trellis"], p(bs.pairs), p(bs.pair_count), None)
    for kw, word in ((dict(cs=None), "null"), (dict(score=None), "null"), (dict(trellis=None), "null"), (dict(beams=0), "beams"),
                     (dict(beams=17), "beams"), (dict(n=0), "n_examples"), (dict(step=4), "step"), (dict(step=-1), "step"),
                     (dict(lp=float("nan")), "length_penalty")):
        rc, msg = advance(**kw)
        assert rc == -1 and "beam_advance" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for t, b in zip((bs.score, bs.rank_of_slot, bs.heap, bs.heap_meta, bs.done, bs.trellis, bs.pairs, bs.cur_len, st), before):
        assert torch.equal(bits(t), bits(b))

    k, vt, _, _ = _caches(False)
    k0, v0 = k.clone(), vt.clone()
    pairs = torch.tensor([[[0, 1]]], dtype=I32, device="cuda")
    cnt = torch.ones((1,), dtype=I32, device="cuda")
    p0 = torch.zeros((6,), dtype=I32, device="cuda")
    pos = torch.full((6,), 9, dtype=I32, device="cuda")

    def copy(**kw):
        a = {**dict(k=p(k), vt=p(vt), klo=None, hd=128, smax=64, pairs=p(pairs), cnt=p(cnt), lists=1, stride=1, p0=p(p0), pos=p(pos), span=9), **kw}
        return _rc(L.llark_kv_copy_slots, a["k"], a["vt"], a["klo"], None, 2, 6, 2, a["hd"], a["smax"], a["pairs"], a["cnt"], a["lists"], a["stride"],
                   a["p0"], a["pos"], a["span"], None)
    for kw in (dict(k=None), dict(pairs=None), dict(cnt=None), dict(p0=None), dict(pos=None), dict(klo=p(k)), dict(hd=64), dict(smax=60),
               dict(lists=0), dict(stride=2000), dict(span=0), dict(span=65)):
        rc, msg = copy(**kw)
        assert rc == -1 and "kv_copy_slots" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(bits(k), bits(k0)) and torch.equal(bits(vt), bits(v0))


# ---- llark_beam_advance ----------------------------------------------------------------------------------------------------------
def _load_ref(ref, bs, state):
    """The reference's state := the device's."""
    B = bs.beams
    ref.score = bs.score.cpu().numpy().copy()
    ref.rank_of_slot = bs.rank_of_slot.cpu().numpy().astype(np.int64)
    ref.done = [bool(x) for x in bs.done.cpu().tolist()]
    ref.cur_len = [int(x) for x in bs.cur_len.cpu().tolist()]
    ref.state = state.cpu().numpy().astype(np.int64)
    heap, meta = bs.heap.cpu().numpy(), bs.heap_meta.cpu().numpy()
    hf = heap.view(np.float32)
    for e in range(bs.n):
        ref.heaps[e] = [dict(score=hf[e, i, 0], sum=hf[e, i, 1], length=int(heap[e, i, 2]), end_step=int(heap[e, i, 3]), end_slot=int(heap[e, i, 4]),
                             arrival=int(heap[e, i, 5]), eos_lp=float(hf[e, i, 6])) for i in range(int(meta[e, 0]))]
        ref.arrivals[e] = int(meta[e, 2])


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return 0 if a == b else abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _same_state(ref, bs, state, step):
    B = bs.beams
    assert bits(bs.score).numpy().tolist() == ref.score.view(np.int32).tolist(), f"step {step}: scores"
    assert bs.rank_of_slot.cpu().tolist() == ref.rank_of_slot.tolist(), f"step {step}: rank_of_slot"
    assert [bool(x) for x in bs.done.cpu().tolist()] == ref.done and bs.cur_len.cpu().tolist() == ref.cur_len, f"step {step}: done / cur_len"
    assert state.cpu().tolist() == ref.state.tolist(), f"step {step}: state"
    heap, meta = bs.heap.cpu().numpy(), bs.heap_meta.cpu().numpy()
    hf, mf = heap.view(np.float32), meta.view(np.float32)
    for e in range(bs.n):
        hs = ref.heaps[e]
        assert int(meta[e, 0]) == len(hs) and int(meta[e, 2]) == ref.arrivals[e], f"step {step}: heap count / arrivals of example {e}"
        assert _ulps(mf[e, 1], ref.worst(e)) <= 1
        for i, h in enumerate(hs):
            assert [int(heap[e, i, j]) for j in (2, 3, 4, 5)] == [h["length"], h["end_step"], h["end_slot"], h["arrival"]], f"step {step} heap {e},{i}"
            assert hf[e, i, 1] == h["sum"] and _ulps(hf[e, i, 0], h["score"]) <= 1
            assert (np.isnan(h["eos_lp"]) and np.isnan(hf[e, i, 6])) or hf[e, i, 6] == np.float32(h["eos_lp"])
    parent, token, lp = ref.trellis[-1]
    tr = bs.trellis[step].cpu().numpy()
    assert tr[:, 0].tolist() == parent.tolist() and tr[:, 1].tolist() == token.tolist(), f"step {step}: trellis"
    got_lp = np.ascontiguousarray(tr[:, 2]).view(np.float32)
    assert all((np.isnan(a) and np.isnan(b)) or a == np.float32(b) for a, b in zip(got_lp, lp))


def _hazard_rule(pairs, parents_before, trellis_row, B):
    """No src is a dst; every dst's old beam had no child; copies = children beyond each parent's first."""
    srcs, dsts = [p[0] for p in pairs], [p[1] for p in pairs]
    assert not set(srcs) & set(dsts) and len(set(dsts)) == len(dsts)
    kids = {}
    for slot, par in enumerate(trellis_row):
        if par >= 0:
            kids.setdefault(int(par), []).append(slot)
    assert all(d not in kids for d in dsts)
    assert len(pairs) == sum(len(v) - 1 for v in kids.values())
    for par, v in kids.items():
        assert par in v                                        # the first child stayed
        assert sorted(d for s, d in pairs if s == par) == sorted(x for x in v if x != par)


@pytest.mark.parametrize("eos_mode", ["frequent", "rare", "off"])
@pytest.mark.parametrize("n_ex", [1, 3])
@pytest.mark.parametrize("beams", [1, 2, 4, 16])
@pytest.mark.parametrize("vocab", [64, 1000])
def test_advance_follows_the_reference_step_by_step(vocab, beams, n_ex, eos_mode):
    steps, eos = 12, (-1 if eos_mode == "off" else 7)
    rng = np.random.default_rng(vocab * 131 + beams * 17 + n_ex)
    table = (2.5 * rng.standard_normal((vocab, vocab))).astype(np.float32)
    if eos >= 0:
        # "frequent": an eos reaches the first B places within the 12 steps in every case (checked with beam_ref alone on the CPU)
        table[:, eos] += (3.5 if vocab == 64 else 6.5) if eos_mode == "frequent" else -1.0
    tab = torch.from_numpy(table).cuda()
    slots = n_ex * beams
    lens = [5 + 3 * e for e in range(n_ex)]
    bs = BeamSearch(n_ex, beams, vocab, steps, "cuda", eos=eos, pad=0, length_penalty=[1.0, 0.6, 2.0][n_ex % 3], early_stopping=(beams == 4))
    bs.admit(lens)
    ref = R.BeamRef(lens, beams, eos, 0, bs.length_penalty, bs.early_stopping)
    state = torch.full((slots,), ops.ROW_ACTIVE, dtype=I32, device="cuda")
    pos = torch.tensor(np.repeat(lens, beams), dtype=I32, device="cuda")
    last = torch.tensor(np.repeat([(11 * e + 3) % vocab for e in range(n_ex)], beams), dtype=I64, device="cuda")
    offs = torch.tensor(np.repeat([5 * e for e in range(n_ex)], beams), dtype=I64, device="cuda")
    closed = 0
    for step in range(steps):
        logits = tab[(last + offs) % vocab].contiguous()
        _load_ref(ref, bs, state)
        pos_before = pos.clone()
        was_done = list(ref.done)
        nxt, done = bs.step(logits, state, pos if step else None)
        want_next, want_pairs = ref.step(cands=(bs.cand_score.cpu().numpy(), bs.cand_token.cpu().numpy().astype(np.int64),
                                                bs.cand_logprob.cpu().numpy().astype(np.float64)))
        _same_state(ref, bs, state, step)
        assert nxt.cpu().tolist() == want_next.tolist() and done == ref.done
        adv = np.repeat([0 if (w or step == 0) else 1 for w in was_done], beams)
        assert (pos.cpu().numpy() - pos_before.cpu().numpy()).tolist() == adv.tolist()
        cnt, pairs = bs.pair_count.cpu().tolist(), bs.pairs.cpu().numpy()
        for e in range(n_ex):
            got = [tuple(int(x) for x in pairs[e, i]) for i in range(cnt[e])]
            assert got == want_pairs[e], f"step {step} example {e}: pairs {got} vs {want_pairs[e]}"
            if not was_done[e] and not ref.done[e]:
                _hazard_rule(got, None, [p if e * beams <= s < (e + 1) * beams else -1 for s, p in enumerate(ref.trellis[-1][0])], beams)
        last = nxt.clone()
        closed = sum(len(h) for h in ref.heaps)
        if all(done):
            break
    if eos_mode == "frequent":
        assert closed > 0
    rseq = min(beams, 2)
    got, want = bs.hypotheses(rseq), ref.finalize(rseq)
    for e in range(n_ex):
        for g, w in zip(got[e], want[e]):
            assert g["tokens"] == w["tokens"] and g["length"] == w["length"] and g["eos"] == w["eos"]
            assert _ulps(g["score"], w["score"]) <= 1 and np.float32(g["sum"]) == np.float32(w["sum"])
            assert [np.float32(x) for x in g["logprobs"]] == [np.float32(x) for x in w["logprobs"]]
            # the score is the sum of the walked log-probabilities over length ** penalty (fp32 accumulation along the path: 1e-5)
            assert g["score"] == pytest.approx(sum(g["logprobs"]) / g["length"] ** bs.length_penalty, rel=1e-5, abs=1e-5)


def test_advance_identical_rows_equal_scores_order_by_rank():
    """Two beams with equal scores whose rows are identical: candidates tie exactly across beams; rank decides, and rank is not slot."""
    V, B = 64, 2
    bs = BeamSearch(1, B, V, 2, "cuda")
    bs.admit([4])
    bs.score.zero_()
    bs.rank_of_slot.copy_(torch.tensor([1, 0], dtype=I32))
    row = torch.zeros((2, V))
    row[:, [9, 30]] = 1.0
    state = torch.full((2,), ops.ROW_ACTIVE, dtype=I32, device="cuda")
    nxt, _ = bs.step(row.cuda(), state)
    # the four best: (rank 0 = slot 1, tok 9), (rank 0, tok 30), (rank 1, tok 9), ...: both live beams are children of slot 1
    assert bs.trellis[0, :, 0].tolist() == [1, 1] and nxt.tolist() == [30, 9] and bs.rank_of_slot.tolist() == [1, 0]
    assert bs.pair_count.tolist() == [1] and bs.pairs[0, 0].tolist() == [1, 0]


# ---- llark_kv_copy_slots ---------------------------------------------------------------------------------------------------------
def _caches(lo, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape_k, shape_v = (2, 6, 2, 64, 128), (2, 6, 2, 128, 64)
    mk = lambda s: torch.randint(-30000, 30000, s, generator=g, dtype=torch.int16).view(torch.bfloat16).cuda()     # noqa: E731
    return mk(shape_k), mk(shape_v), (mk(shape_k) if lo else None), (mk(shape_v) if lo else None)


@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("span", [1, 7, 8, 9, 33])
@pytest.mark.parametrize("p0", [0, 8, 24])
def test_kv_copy_slots_moves_exactly_the_span(p0, span, lo):
    n = p0 + span
    up = (n + 7) // 8 * 8
    lists = {"fan out": ([[1, 0], [1, 3], [1, 5]], 3), "two sources": ([[0, 2], [4, 5], [4, 1]], 3), "count 0": ([[1, 0], [1, 3]], 0),
             "longer than the count": ([[2, 0], [2, 4], [3, 5], [3, 1]], 2)}
    for name, (pairs, count) in lists.items():
        k, vt, klo, vlo = _caches(lo, seed=p0 + span)
        before = [None if t is None else t.clone() for t in (k, vt, klo, vlo)]
        pos = torch.full((6,), n, dtype=I32, device="cuda")
        p0s = torch.full((6,), p0, dtype=I32, device="cuda")
        ops.kv_copy_slots(k, vt, torch.tensor([pairs], dtype=I32, device="cuda"), torch.tensor([count], dtype=I32, device="cuda"), p0s, pos,
                          span, klo, vlo)
        for t, b, is_v in ((k, before[0], False), (vt, before[1], True), (klo, before[2], False), (vlo, before[3], True)):
            if t is None:
                continue
            want = b.clone()
            free = torch.zeros_like(b, dtype=torch.bool)               # [n, up) of a destination's V^T rows may be overwritten
            for s, d in pairs[:count]:
                if is_v:
                    want[:, d, :, :, p0:n] = b[:, s, :, :, p0:n]
                    free[:, d, :, :, n:up] = True
                else:
                    want[:, d, :, p0:n] = b[:, s, :, p0:n]
            same = (bits(t) == bits(want)) | free.cpu()
            assert bool(same.all()), f"{name}: {int((~same).sum())} elements differ"
        if count == 0:
            assert all(t is None or torch.equal(bits(t), bits(b)) for t, b in zip((k, vt, klo, vlo), before))


def test_kv_copy_slots_refuses_bad_entries_on_the_device():
    """Entries the kernel must not act on: a slot out of range, src == dst, a p0 that is no multiple of 8, an empty span, a span above
    max_span.  Nothing moves; one good entry in a second list does."""
    k, vt, _, _ = _caches(False, 4)
    k0, v0 = k.clone(), vt.clone()
    pairs = torch.tensor([[[0, 6], [-1, 2], [3, 3], [0, 1], [0, 2], [0, 4]], [[5, 3], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]]], dtype=I32, device="cuda")
    cnt = torch.tensor([6, 1], dtype=I32, device="cuda")
    p0 = torch.tensor([0, 4, 16, 8, 0, 0], dtype=I32, device="cuda")         # dst 1: p0 = 4; dst 2: p0 = 16 >= len 12: empty
    pos = torch.tensor([12, 12, 12, 12, 12, 20], dtype=I32, device="cuda")   # dst 4 from src 0: span 12 > max_span 10
    ops.kv_copy_slots(k, vt, pairs, cnt, p0, pos, 12)
    want_k, want_v = k0.clone(), v0.clone()
    want_k[:, 4, :, 0:12], want_v[:, 4, :, :, 0:16] = k0[:, 0, :, 0:12], v0[:, 0, :, :, 0:16]      # max_span 12 takes (0, 4)
    want_k[:, 3, :, 8:20], want_v[:, 3, :, :, 8:24] = k0[:, 5, :, 8:20], v0[:, 5, :, :, 8:24]
    assert torch.equal(bits(k), bits(want_k)) and torch.equal(bits(vt), bits(want_v))
    k.copy_(k0), vt.copy_(v0)
    ops.kv_copy_slots(k, vt, pairs[:1].contiguous(), cnt[:1].contiguous(), p0, pos, 10)
    assert torch.equal(bits(k), bits(k0)) and torch.equal(bits(vt), bits(v0))
