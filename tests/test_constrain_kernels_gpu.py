"""GPU: llark_constrain_rows and llark_beam_topk_rows_banned (csrc/constrain.hip, csrc/beam.hip) against tests/constrain_ref.py.

Everything the constraint kernel writes is integers or copied bits, so every comparison is exact: the processed rows (raw bits or
-inf), the bitmap, the counts, the histories and their lengths.  The banned top-k must give the reference's candidates over the unbanned
columns with log-probabilities that keep the bits of llark_token_logprob_rows."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import constrain_ref as CR
from kernel_util import bits
from llark_amd import _lib, ops

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
N, W, EOS = 3, 320, 4                     # n-gram size, history width, eos
WORDS = [[2], [1, 3], [0, 1, 5], [3, 3, 3, 3], [EOS]]
LENGTHS = [0, N - 2, N - 1, N, 300, W - 1, W]           # per slot, cycled: full at W
SENT = -777.25


@functools.lru_cache(maxsize=None)
def _rows(vocab, rows):
    from logprob_ref import make_rows
    x = make_rows(vocab, rows, 3)
    x.setflags(write=False)
    return x


def _histories(slots, vocab, seed):
    """Histories over a six-token alphabet, so that n-grams and the words recur, with ids of -1 and >= vocab sprinkled in."""
    rng = np.random.default_rng(seed)
    hists, plens, last = [], [], []
    for s in range(slots):
        L = LENGTHS[s % len(LENGTHS)]
        h = rng.integers(0, 6, size=L)
        odd = rng.random(L) < 0.05
        h = np.where(odd, rng.choice([-1, vocab, vocab + 5], size=L), h)
        hists.append([int(t) for t in h])
        plens.append(int(rng.integers(0, L + 1)))
        last.append(int(rng.choice([0, 1, 2, 3, 5, -1, vocab])) if s % 5 else int(rng.integers(0, 6)))
    return hists, plens, last


def _device_state(hists, plens, guard=64):
    """hist [slots, W] inside a guarded buffer (what lies before and behind the rows must not change), hist_len, prompt_len."""
    slots = len(hists)
    buf = torch.full((guard + slots * W + guard,), -5, dtype=I32)
    hist = buf[guard:guard + slots * W].view(slots, W)
    for s, h in enumerate(hists):
        hist[s, :len(h)] = torch.tensor(h, dtype=I32)
        hist[s, len(h):] = -3 - s
    buf = buf.cuda()
    return buf, buf[guard:guard + slots * W].view(slots, W), torch.tensor([len(h) for h in hists], dtype=I32).cuda(), torch.tensor(plens, dtype=I32).cuda()


def _table(words):
    offs = [0]
    for w in words:
        offs.append(offs[-1] + len(w))
    return torch.tensor([t for w in words for t in w], dtype=I32).cuda(), torch.tensor(offs, dtype=I32).cuda()


@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("vocab", [33, 70, 32003, 50435])
def test_constrain_rows_against_the_reference(vocab, rows):
    logits = _rows(vocab, rows)
    slots = rows + 6
    hists, plens, last = _histories(slots, vocab, 11 * vocab + rows)
    perm = np.random.default_rng(rows).permutation(slots)[:rows].astype(np.int32)
    state = np.full(slots, ops.ROW_ACTIVE, dtype=np.int32)
    if rows >= 3:
        perm[1] = -1                                               # a row without a slot
        state[perm[2]] = ops.ROW_FINISHED
    if rows == 64:
        perm[5] = slots                                            # a slot past the end
        state[perm[7]] = ops.ROW_IDLE
    min_new, min_len = 2, 4
    words = CR.words_of(WORDS[:-1], [WORDS[-1][0]], EOS)          # the [eos] word is dropped on the host, as DeviceConstraints does
    assert [EOS] not in words

    ldl = (vocab + 63) // 64 * 64 + 64
    dev = torch.full((rows, ldl), 1e9, dtype=F32)
    dev[:, :vocab] = torch.from_numpy(np.ascontiguousarray(logits))
    dev = dev.cuda()
    ldo = vocab + 5
    out = torch.full((rows, ldo), SENT, dtype=F32, device="cuda")
    nwords = (vocab + 31) // 32
    ban = torch.full((slots, nwords + 1), 0x5A5A5A5A, dtype=I32, device="cuda")
    nb = torch.full((rows,), -9, dtype=I32, device="cuda")
    status = torch.zeros((1,), dtype=I32, device="cuda")
    buf, hist, hlen, plen = _device_state(hists, plens)
    before = buf.clone()
    bw_t, bw_o = _table(words)
    ops.constrain_rows(dev, vocab=vocab, state=torch.from_numpy(state).cuda(), slot_of_row=torch.from_numpy(perm).cuda(), hist=hist,
                       hist_len=hlen, prompt_len=plen, last_token=torch.tensor(last, dtype=I64).cuda(), no_repeat_ngram_size=N, bw_tokens=bw_t,
                       bw_off=bw_o, eos=EOS, min_new_tokens=min_new, min_length=min_len, out=out, ban=ban, n_banned=nb, status=status)

    served = {int(perm[r]): r for r in range(rows) if 0 <= perm[r] < slots and state[perm[r]] == ops.ROW_ACTIVE}
    active = [s in served for s in range(slots)]
    new, full = CR.update_history(hists, None, last, active, width=W)
    assert full == any(active[s] and len(hists[s]) == W for s in range(slots))
    assert int(status.item()) == (ops.CONSTRAIN_STATUS_FULL if full else 0)
    want_buf = before.cpu().clone()
    want_hist = want_buf[64:64 + slots * W].view(slots, W)
    for s in range(slots):
        if active[s] and len(new[s]) > len(hists[s]):
            want_hist[s, len(hists[s])] = max(-1, min(new[s][-1], 2 ** 31 - 1))
    assert torch.equal(buf.cpu(), want_buf), "history rows (or what lies around them) differ"
    assert hlen.cpu().tolist() == [len(h) for h in new]

    h_out, h_ban, h_nb = out.cpu(), ban.cpu(), nb.cpu()
    n_nonempty = 0
    for r in range(rows):
        s = int(perm[r])
        if s not in served or served[s] != r:
            assert bool((h_out[r] == SENT).all()) and int(h_nb[r]) == -9, f"skipped row {r} was written"
            continue
        banned = CR.banned_set(new[s], vocab, n=N, words=words, eos=EOS, prompt_len=plens[s], min_new=min_new, min_len=min_len)
        n_nonempty += bool(banned)
        want = torch.from_numpy(CR.processed_row(logits[r], banned))
        assert torch.equal(bits(h_out[r, :vocab]), bits(want)), f"row {r} (slot {s}, history {len(new[s])})"
        assert bool((h_out[r, vocab:] == SENT).all()), f"row {r}: columns past the vocabulary were written"
        assert torch.equal(h_ban[s, :nwords], torch.from_numpy(CR.bitmap(banned, vocab))) and int(h_ban[s, nwords]) == 0x5A5A5A5A
        assert int(h_nb[r]) == len(banned)
    for s in range(slots):
        if s not in served:
            assert bool((h_ban[s] == 0x5A5A5A5A).all()), f"bitmap of slot {s}, which no row serves, was written"
    assert n_nonempty >= 1


@pytest.mark.parametrize("vocab", [33, 32003])
def test_constrain_rows_without_state_or_slot_table_and_single_outputs(vocab):
    """state=None, slot_of_row=None: row r is slot r.  Each output alone gives what it gives among the others; a prefill launch
    (no last token) leaves the histories as they are."""
    rows = 7
    logits = _rows(vocab, rows)
    hists, plens, _ = _histories(rows, vocab, 5 + vocab)
    words = CR.words_of(WORDS, (), EOS)
    dev = torch.from_numpy(np.ascontiguousarray(logits)).cuda()           # ldl = vocab: odd, rows at every alignment
    bw_t, bw_o = _table(words)
    buf, hist, hlen, plen = _device_state(hists, plens)
    before = buf.clone()
    kw = dict(vocab=vocab, hist=hist, hist_len=hlen, prompt_len=plen, no_repeat_ngram_size=N, bw_tokens=bw_t, bw_off=bw_o, eos=EOS,
              min_new_tokens=1, min_length=0)
    out = torch.full((rows, vocab), SENT, dtype=F32, device="cuda")
    ops.constrain_rows(dev, out=out, **kw)
    ban = torch.zeros((rows, (vocab + 31) // 32), dtype=I32, device="cuda")
    ops.constrain_rows(dev, ban=ban, **kw)
    nb = torch.zeros((rows,), dtype=I32, device="cuda")
    ops.constrain_rows(dev, n_banned=nb, **kw)
    assert torch.equal(buf, before) and hlen.cpu().tolist() == [len(h) for h in hists]
    for r in range(rows):
        banned = CR.banned_set(hists[r], vocab, n=N, words=words, eos=EOS, prompt_len=plens[r], min_new=1)
        assert torch.equal(bits(out[r]), bits(torch.from_numpy(CR.processed_row(logits[r], banned)))), f"row {r}"
        assert torch.equal(ban[r].cpu(), torch.from_numpy(CR.bitmap(banned, vocab))) and int(nb[r]) == len(banned)
    # no history at all: only the one-token words and the EOS rule can ban
    out2 = torch.full((rows, vocab), SENT, dtype=F32, device="cuda")
    ops.constrain_rows(dev, vocab=vocab, bw_tokens=bw_t, bw_off=bw_o, eos=EOS, min_new_tokens=1, out=out2)
    banned = CR.banned_set([], vocab, words=words, eos=EOS, min_new=1)
    assert banned == {2, EOS}
    for r in range(rows):
        assert torch.equal(bits(out2[r]), bits(torch.from_numpy(CR.processed_row(logits[r], banned))))


def test_ngram_sizes_1_to_64_on_a_long_history():
    vocab, L = 70, 2047
    rng = np.random.default_rng(8)
    base = rng.integers(0, 4, size=L).tolist()
    sizes = [1, 2, 5, 33, 64]
    hists = []
    for n in sizes:                                                # make the last n - 1 tokens recur earlier, followed by token 9
        h = list(base)
        if n > 1:
            tail = h[L - (n - 1):]
            h[100:100 + n - 1] = tail
            h[100 + n - 1] = 9
        hists.append(h)
    dev = torch.from_numpy(np.ascontiguousarray(_rows(vocab, 1))).cuda()
    for n, h in zip(sizes, hists):
        hist = torch.tensor([h + [0]], dtype=I32).cuda()
        hlen = torch.tensor([L], dtype=I32).cuda()
        ban = torch.zeros((1, 3), dtype=I32, device="cuda")
        ops.constrain_rows(dev, hist=hist, hist_len=hlen, no_repeat_ngram_size=n, ban=ban)
        want = CR.banned_set(h, vocab, n=n)
        assert n == 1 or 9 in want
        assert torch.equal(ban[0].cpu(), torch.from_numpy(CR.bitmap(want, vocab))), f"n = {n}"


def test_fork_pattern_of_a_beam_step_in_place():
    """Four beams, two examples: parents and tokens from BeamRef steps; the histories follow the beams, in place, from the trellis'
    parent column passed as it lies (stride 3)."""
    vocab, B, prompts = 70, 4, [[1, 2, 3, 1, 2], [4, 4]]
    ref = CR.ConstrainedBeamRef(prompts, B, vocab, n=2)
    slots = len(prompts) * B
    hists = [list(prompts[s // B]) for s in range(slots)]
    buf, hist, hlen, plen = _device_state(hists, [len(h) for h in hists])
    rng = np.random.default_rng(2)
    forked = 0
    ban = torch.zeros((slots, 3), dtype=I32, device="cuda")
    for step in range(5):
        logits = R.make_rows(vocab, slots, 20 + step)
        dev = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
        if step == 0:
            ops.constrain_rows(dev, hist=hist, hist_len=hlen, prompt_len=plen, no_repeat_ngram_size=2, ban=ban)
        else:
            parent, token, _ = ref.ref.trellis[-1]
            forked += int((parent != np.arange(slots)).sum())
            trellis = torch.tensor(np.stack([parent, token, np.zeros(slots)], axis=1), dtype=I32).cuda()
            ops.constrain_rows(dev, hist=hist, hist_len=hlen, prompt_len=plen, parent=trellis[:, 0], last_token=torch.from_numpy(ref.last).cuda(),
                               no_repeat_ngram_size=2, ban=ban)
        ref.step(logits)
        got_len = hlen.cpu().tolist()
        for s in range(slots):
            assert got_len[s] == len(ref.hists[s]) and hist[s, :got_len[s]].cpu().tolist() == ref.hists[s], f"step {step}, slot {s}"
            banned = CR.banned_set(ref.hists[s], vocab, n=2)
            assert torch.equal(ban[s].cpu(), torch.from_numpy(CR.bitmap(banned, vocab)))
    assert forked >= 4
    for s in range(slots):                                         # a slot's history is its beam's: prompt + the trellis' backtrack
        assert ref.hists[s] == prompts[s // B] + ref.ref.backtrack(ref.ref.steps - 1, s)[0]


def test_refusals():
    x = torch.zeros((1, 65537), dtype=F32, device="cuda")
    out = torch.zeros((1, 65537), dtype=F32, device="cuda")
    with pytest.raises(_lib.LlarkHipError, match="above 65536"):
        ops.constrain_rows(x, out=out)
    x, out = x[:, :64].contiguous(), out[:, :64].contiguous()
    L = _lib.lib()
    hist = torch.zeros((1, 8), dtype=I32, device="cuda")
    hlen = torch.zeros((1,), dtype=I32, device="cuda")

    def call(**kw):
        a = dict(logits=x.data_ptr(), ldl=64, vocab=64, rows=1, slots=1, state=None, slot_of_row=None, hist=hist.data_ptr(), ld_hist=8,
                 hist_len=hlen.data_ptr(), prompt_len=None, parent=None, parent_stride=1, last_token=None, n=0, bw_tokens=None, bw_off=None,
                 n_words=0, bw_total=0, eos=-1, min_new=0, min_len=0, out=out.data_ptr(), ldo=64, ban=None, ld_ban=0, n_banned=None, status=None)
        a.update(kw)
        return L.llark_constrain_rows(*a.values(), None)
    assert call() == 0
    for bad, word in ((dict(logits=None), "null"), (dict(out=None), "null"), (dict(ldl=63), "ldl"), (dict(n=65), "no_repeat_ngram"),
                      (dict(n=-1), "no_repeat_ngram"), (dict(hist_len=None), "hist_len"), (dict(hist=None), "hist"), (dict(ld_hist=0), "ld_hist"),
                      (dict(hist=None, hist_len=None, n=2), "without hist"), (dict(n_words=4097, bw_total=4097), "caps"),
                      (dict(n_words=2, bw_total=1), "caps"), (dict(n_words=1, bw_total=1), "bw_tokens"), (dict(min_new=-1), "min_new_tokens"),
                      (dict(ldo=63), "ldo"), (dict(ban=out.data_ptr(), ld_ban=1), "ld_ban"), (dict(rows=2), "rows"),
                      (dict(parent=hlen.data_ptr(), parent_stride=0), "parent_stride")):
        assert call(**bad) == -1, bad
        assert word in L.llark_last_error().decode(), (bad, L.llark_last_error().decode())


@functools.lru_cache(maxsize=None)
def _beam_case(vocab, beams):
    """8 rows of beam_ref.make_rows, scores, and per row a banned set that takes out its two best tokens, the fourth best and 40
    random ones; row 7 keeps fewer than 2B tokens.  The reference's 2B + 1 best unbanned candidates and the count of near ties."""
    rows = 8
    logits = R.make_rows(vocab, rows, 0)
    rng = np.random.default_rng(vocab + beams)
    score = rng.uniform(-20.0, 0.0, rows).astype(np.float32)
    bans, refs, near = [], [], 0
    for r in range(rows):
        _, t, _ = R.row_candidates(logits[r], score[r], beams, 4)
        ban = {int(t[0]), int(t[1]), int(t[3])} | {int(x) for x in rng.choice(vocab, size=min(40, vocab // 2), replace=False)}
        if r == 7:
            ban = set(range(vocab)) - {int(x) for x in rng.choice(vocab, size=2 * beams - 1, replace=False)}
        bans.append(ban)
        c, tk, lp = R.row_candidates(logits[r], score[r], beams, count=vocab)
        keep = [i for i in range(vocab) if int(tk[i]) not in ban][:2 * beams + 1]
        c, tk = c[keep], tk[keep]
        tol = R.cand_tols(logits[r], score[r], tk, c)
        d = np.abs(np.diff(c))
        near += int(((d > 0) & (d <= tol[:-1] + tol[1:])).sum())
        refs.append(CR.banned_candidates(logits[r], score[r], beams, ban))
    logits.setflags(write=False)
    return logits, score, bans, refs, near


@pytest.mark.parametrize("vocab, beams", [(70, 3), (32003, 3), (50435, 16), (51201, 1)])
def test_beam_topk_rows_banned(vocab, beams):
    logits, score, bans, refs, near = _beam_case(vocab, beams)
    assert near == 0, "the inputs hold a near tie: choose another seed"
    rows, K = logits.shape[0], 2 * beams
    dev = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    sc = torch.from_numpy(score).cuda()
    ban = torch.from_numpy(np.stack([CR.bitmap(b, vocab) for b in bans])).cuda()

    def outs():
        return (torch.full((rows, K), SENT, dtype=F32, device="cuda"), torch.full((rows, K), -9, dtype=I32, device="cuda"),
                torch.full((rows, K), SENT, dtype=F32, device="cuda"))
    cs, ct, cl = outs()
    fb = torch.zeros((1,), dtype=I32, device="cuda")
    ops.beam_topk_rows(dev, sc, beams, cs, ct, cl, fallbacks=fb, ban=ban)
    assert int(fb.item()) == 0
    hs, ht, hl = cs.cpu().numpy(), ct.cpu().numpy(), cl.cpu().numpy()
    for r in range(rows):
        c, t, lp = refs[r]
        assert ht[r].tolist() == t.tolist(), f"row {r}: tokens {ht[r].tolist()} vs {t.tolist()}"
        assert not set(ht[r].tolist()) & bans[r]
        live = t >= 0
        tol = R.cand_tols(logits[r], score[r], t[live], c[live])
        assert (np.abs(hs[r][live].astype(np.float64) - c[live]) <= tol).all()
        assert (hs[r][live] == (score[r] + hl[r][live]).astype(np.float32)).all()
        assert np.isneginf(hs[r][~live]).all() and np.isneginf(hl[r][~live]).all()
    assert (refs[7][1] < 0).sum() == 1                             # the row with 2B - 1 tokens left: one empty place
    # the candidates' log-probabilities: the bits of llark_token_logprob_rows on the raw row -- a banned token still counts in the sum
    for k in range(K):
        toks = ct[:, k].to(I64).contiguous()
        want = ops.token_logprob_rows(dev, toks, torch.full((rows,), float("-inf"), dtype=F32, device="cuda"))
        assert torch.equal(bits(want), bits(cl[:, k].contiguous())), f"candidate {k}"
    # an all-zero bitmap: the bits of the unbanned entry point
    a = outs()
    b = outs()
    ops.beam_topk_rows(dev, sc, beams, *a, ban=torch.zeros_like(ban))
    ops.beam_topk_rows(dev, sc, beams, *b)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
