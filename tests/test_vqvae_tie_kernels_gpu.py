"""GPU: the near-tie certificate (csrc/vqvae.hip: llark_codebook_argmin_tie) against float64 distances, and the exact fix-up
(llark_vqvae_fix_near_ties) against the exact encoder, at the kernel level.

The rule: a token is flagged <=> second-best distance - best distance < thr = |x| (tie_a sqrt(d_best) + tie_b |x|).

  * planted near-ties: codes k_b = k_a + eps and a token at (k_a + k_b) / 2 + alpha (k_a - k_b), alpha solved in float64 so that the gap
    is 0.5 thr (must be flagged) or 2 thr (must not be); |eps| ~ |x| so that d_best is far above the fp32 noise of a distance and the
    realised ratio after rounding the token to fp32 stays in [0.4, 0.6] / [1.8, 2.2] (asserted).  a and b sit in the same group of 8
    codes (one unrolled step of the scan), in different groups of the same quarter (one wave), and in every ordered pair of quarters
    (the cross-wave merge), in both index orders: a threshold wrong by 2 x, or a second-best lost in a merge, fails.
  * random tokens: flagged <=> gap < thr in float64, except within the fp32 rounding of the two distance chains,
    |gap - thr| <= 2 * 70 * 2^-24 (|x| + max|k|)^2 + 4 * 2^-24 thr (64 fmaf steps and a few roundings per distance, two distances; the
    threshold's own three roundings), where either answer is accepted; that band may take at most 1 % of the tokens."""
import pytest
import torch

import kernel_util as U

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
INT_SENTINEL = -77777777


def _quantities(x, k, tie_a, tie_b):
    """float64, per token [n][t]: best and second-best squared distance, |x|, threshold, rounding band"""
    xd = x.double().permute(0, 2, 1)                                        # [n][t][64]
    d = ((xd[:, :, None, :] - k.double()[None, None]) ** 2).sum(-1) if k.shape[0] <= 64 else None
    if d is None:
        d = (xd ** 2).sum(-1, keepdim=True) - 2.0 * xd @ k.double().t() + (k.double() ** 2).sum(-1)[None, None]
    two = torch.topk(d, 2, dim=-1, largest=False).values
    best, second = two[..., 0].clamp_min(0.0), two[..., 1]
    xn = (xd ** 2).sum(-1).sqrt()
    thr = xn * (tie_a * best.sqrt() + tie_b * xn)
    band = 2 * 70 * EPS24 * (xn + float(k.double().norm(dim=1).max())) ** 2 + 4 * EPS24 * thr
    return best, second, xn, thr, band


def _pairs(bins):
    """(a, b) code pairs: same group of 8, same quarter / different groups (where a quarter has two groups), every ordered pair of
    quarters; both index orders; every code used once"""
    per = bins // 4
    free = [list(range(q * per, (q + 1) * per)) for q in range(4)]
    out = []

    def take(q, group=None):
        for i in free[q]:
            if group is None or i // 8 == group:
                free[q].remove(i)
                return i
        raise AssertionError("no free code")

    for q, flip in ((0, False), (1, True)):                                 # same group of 8
        a = take(q)
        b = take(q, a // 8)
        out.append(("group", b, a) if flip else ("group", a, b))
    if per >= 16:
        for q, flip in ((2, False), (3, True)):                             # same wave, another group
            a = take(q)
            b = next(i for i in free[q] if i // 8 != a // 8)
            free[q].remove(b)
            out.append(("quarter", b, a) if flip else ("quarter", a, b))
    for qa in range(4):
        for qb in range(4):
            if qa != qb:
                out.append((f"q{qa}->q{qb}", take(qa), take(qb)))
    return out


def _plant(k, x, slots, tie_a, tie_b, g):
    """writes the pairs into k and two tokens per pair into x (slots: (n, tok) positions); returns {(n, tok): (must_flag, label)}"""
    want = {}
    pairs = _pairs(k.shape[0])
    assert len(slots) >= 2 * len(pairs)
    for label, a, b in pairs:
        k[b] = k[a] + torch.randn(64, generator=g)                          # |eps| ~ 8 ~ |x|
    it = iter(slots)
    for label, a, b in pairs:
        ka, kb = k[a].double(), k[b].double()
        e2 = float(((ka - kb) ** 2).sum())
        for ratio in (0.5, 2.0):
            alpha = 0.0
            for _ in range(30):                                             # gap = 2 alpha |eps|^2 = ratio thr(alpha)
                xv = (ka + kb) / 2 + alpha * (ka - kb)
                xn = float(xv.norm())
                alpha = ratio * xn * (tie_a * (0.5 - alpha) * e2 ** 0.5 + tie_b * xn) / (2 * e2)
            assert 0 < alpha < 0.25
            n, tok = next(it)
            x[n, :, tok] = ((ka + kb) / 2 + alpha * (ka - kb)).float()
            want[(n, tok)] = (ratio < 1, f"{label} a={a} b={b} ratio {ratio}", a)
    return want


def _run(x, k, tie_a, tie_b, cap=None, slack=8):
    """-> codes [n][t], count, the list buffer (CPU, with its slack), reference codes of ops.codebook_argmin"""
    from llark_amd import ops
    n, _, t = x.shape
    cap = n * t + 3 if cap is None else cap
    xd, kd = x.cuda(), k.cuda()
    kk = ops.codebook_norms(kd)
    count = torch.full((1,), 123, dtype=torch.int32, device="cuda")        # the call zeroes it
    lst = torch.full((cap + slack,), INT_SENTINEL, dtype=torch.int32, device="cuda")
    codes = ops.codebook_argmin_tie(xd, kd, kk, tie_a, tie_b, count, lst[:cap])
    ref = ops.codebook_argmin(xd, kd, kk)
    torch.cuda.synchronize()
    return codes.cpu(), int(count.item()), lst.cpu(), ref.cpu()


def _check_list(lst, count, cap, must, may, total):
    """the first min(count, cap) entries are distinct valid ids of tokens that must or may be flagged; the rest is untouched"""
    stored = lst[:min(count, cap)].tolist()
    assert len(set(stored)) == len(stored), "a token id is listed twice"
    assert all(0 <= i < total for i in stored) and set(stored) <= must | may, sorted(set(stored) - must - may)[:10]
    assert bool((lst[min(count, cap):] == INT_SENTINEL).all()), "the list was written beyond min(count, cap)"
    return set(stored)


SHAPES = [(bins, t, n) for bins in (32, 64, 2048) for t in (1, 63, 64, 65, 300) for n in (1, 3)]


@pytest.mark.parametrize("bins,t,n", SHAPES)
def test_flags_against_float64(bins, t, n):
    ci = SHAPES.index((bins, t, n))
    tie_a, tie_b = (0.005, 0.02, 0.05)[ci % 3], (12.0, 100.0)[ci % 2] * 2.0 ** -23
    g = torch.Generator().manual_seed(1000 + ci)
    k = torch.randn(bins, 64, generator=g)
    x = torch.randn(n, 64, t, generator=g)
    want = {}
    if n * t >= 2 * 16:                                                     # room for two tokens per planted pair
        perm = torch.randperm(n * t, generator=g)[:2 * 16].tolist()
        if t >= 64:                                                         # ... the last lane of a block and the clip's last token among them
            perm = list(dict.fromkeys([63, n * t - 1] + perm))[:2 * 16]
        want = _plant(k, x, [divmod(i, t) for i in perm], tie_a, tie_b, g)
    best, second, xn, thr, band = _quantities(x, k, tie_a, tie_b)
    gap = second - best
    excluded = (gap - thr).abs() <= band
    must = {int(i) for i in ((gap < thr) & ~excluded).flatten().nonzero().flatten()}
    may = {int(i) for i in excluded.flatten().nonzero().flatten()}
    for (nn, tok), (flag, label, a) in want.items():
        r = float(gap[nn, tok] / thr[nn, tok])
        assert (0.4 <= r <= 0.6) if flag else (1.8 <= r <= 2.2), f"planted {label}: realised gap / thr {r:.3f}"
        assert not bool(excluded[nn, tok]) and ((nn * t + tok) in must) == flag
    codes, count, lst, ref = _run(x, k, tie_a, tie_b)
    share = len(may) / (n * t)
    print(f"\n[tie] bins {bins} t {t} n {n} tie_a {tie_a} tie_b {tie_b:.2e}: flagged {count} of {n * t} ({len(must)} certain, {len(want)} planted), "
          f"excluded share {share:.4f}")
    assert share <= 0.01
    assert torch.equal(codes, ref), "codes differ from llark_codebook_argmin"
    for (nn, tok), (flag, label, a) in want.items():
        assert int(codes[nn, tok]) == a, f"planted {label}: code {int(codes[nn, tok])}"
    stored = _check_list(lst, count, n * t + 3, must, may, n * t)
    assert len(stored) == count, f"flag_count {count} but {len(stored)} ids listed"
    missing = must - stored
    bad = [want[divmod(i, t)][1] for i in missing if divmod(i, t) in want]
    assert not missing, f"{len(missing)} tokens below the threshold were not flagged, planted among them: {bad}"


def test_list_capacity_and_counter():
    """about 40 flagged, room for 5: the counter keeps counting, five distinct valid ids are stored, nothing beyond cap is written"""
    g = torch.Generator().manual_seed(5)
    k, x = torch.randn(2048, 64, generator=g), torch.randn(2, 64, 150, generator=g)
    best, second, xn, thr, band = _quantities(x, k, 0.01, 12 * 2.0 ** -23)
    excluded = ((second - best) - thr).abs() <= band
    must = {int(i) for i in (((second - best) < thr) & ~excluded).flatten().nonzero().flatten()}
    may = {int(i) for i in excluded.flatten().nonzero().flatten()}
    assert 25 <= len(must) <= 60 and len(may) <= 3, (len(must), len(may))
    codes, count, lst, ref = _run(x, k, 0.01, 12 * 2.0 ** -23, cap=5)
    print(f"\n[tie] cap 5: counted {count}, certain {len(must)}, excluded {len(may)}")
    assert len(must) <= count <= len(must) + len(may) and torch.equal(codes, ref)
    assert len(_check_list(lst, count, 5, must, may, 300)) == 5


def test_duplicates_zero_threshold_nan_and_refusals():
    from llark_amd import _lib, ops
    g = torch.Generator().manual_seed(6)
    k, x = torch.randn(2048, 64, generator=g), torch.randn(2, 64, 70, generator=g)
    k[1500] = k[77]                                                         # an exact duplicate in another quarter of the codebook
    x[0, :, 10] = k[77]                                                     # a token on it
    x[1, :, 69] = k[77] + 0.01 * torch.randn(64, generator=g)               # and one next to it: both distances are the same bits
    codes, count, lst, ref = _run(x, k, 0.0, 1e-20)                         # any positive threshold
    assert torch.equal(codes, ref) and int(codes[0, 10]) == 77 and int(codes[1, 69]) == 77, "an exact tie goes to the lower index"
    assert count == 2 and set(lst[:2].tolist()) == {10, 70 + 69} and bool((lst[2:] == INT_SENTINEL).all())
    codes, count, lst, ref = _run(x, k, 0.0, 0.0)                           # zero threshold: nothing finite is flagged
    assert count == 0 and bool((lst == INT_SENTINEL).all()) and torch.equal(codes, ref)
    x[1, 5, 3] = float("nan")                                               # a NaN channel: flagged, as the kernel promises
    for ta, tb in ((0.0, 0.0), (0.01, 1e-6)):
        codes, count, lst, ref = _run(x, k, ta, tb)
        assert (70 + 3) in lst[:count].tolist() and torch.equal(codes, ref)
    kd, xd = k.cuda(), x.cuda()
    cnt, fl = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    for ta, tb in ((-1e-3, 0.0), (0.0, -1e-9)):
        with pytest.raises(_lib.LlarkHipError, match="negative"):
            ops.codebook_argmin_tie(xd, kd, ops.codebook_norms(kd), ta, tb, cnt, fl)


# ---------------------------------------------------------------------------------------------------------------------
# llark_vqvae_fix_near_ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_exact():
    from llark_amd.jukebox.hparams import hparams_tiny
    from llark_amd.jukebox.synthetic import init_codebook_from_encodings, make_vqvae_weights
    from llark_amd.jukebox.vqvae import VQVAE
    hps = hparams_tiny()
    w = make_vqvae_weights(hps, 0)
    g = torch.Generator().manual_seed(21)
    t = torch.arange(hps.sample_length) / 44100.0
    audio = torch.stack([0.5 * torch.sin(2 * torch.pi * f * t) for f in (220.0, 587.0)]) + 0.1 * torch.randn(2, hps.sample_length, generator=g)
    audio = audio.float().cuda().contiguous()
    vq = VQVAE(hps, w, "cuda", exact=True)
    enc = vq.encoder_forward(audio[:, None, :])
    vq.set_codebook(init_codebook_from_encodings(enc.permute(1, 0, 2).reshape(enc.shape[1], -1).cpu(), hps.l_bins))
    ref = vq.encode_top(audio)
    assert ref.shape == (2, hps.n_ctx) and len(ref.unique()) > 50
    return hps, vq, audio, ref


def _fix(vq, audio, ids, count, halo, win, codes):
    from llark_amd import ops
    r2t = vq.hps.raw_to_tokens
    wlen, m = win * r2t, max(len(ids), 1)
    width = max(layer[1].shape[2] for layer in vq.layers)
    dev = audio.device
    fl = torch.tensor(ids if ids else [0], dtype=torch.int32, device=dev)
    bufs = [torch.empty((m * width * (wlen // 2 + 1),), dtype=torch.float32, device=dev) for _ in range(2)]
    ops.vqvae_fix_near_ties(vq._plan(), audio, r2t, fl, count, halo, win, torch.empty((m * wlen,), dtype=torch.float32, device=dev),
                            torch.empty((m,), dtype=torch.int32, device=dev), bufs[0], bufs[1], vq.k, vq.kk, codes)
    torch.cuda.synchronize()


def test_fix_near_ties_patches_exactly_the_listed_tokens(tiny_exact):
    from llark_amd import _lib
    hps, vq, audio, ref = tiny_exact
    t, halo, win = hps.n_ctx, vq.halo_tokens, vq.win_tokens
    assert 2 * halo + 1 <= win < t
    # windows clamped to either clip end, on both sides of where the clamping starts, and in the interior
    toks = [0, halo - 1, halo, halo + 1, t // 2 - 5, t - win + halo - 1, t - win + halo, t - win + halo + 1, t - 1]
    ids = [c * t + tok for c in range(2) for tok in toks]
    ids.insert(4, ids[1])                                                   # one id twice
    codes = torch.full((2, t), -1, dtype=torch.int64, device="cuda")
    _fix(vq, audio, ids, len(ids), halo, win, codes)
    flat, want = codes.flatten().cpu(), torch.full((2 * t,), -1, dtype=torch.int64)
    want[ids] = ref.flatten().cpu()[ids]
    assert torch.equal(flat, want), f"{int((flat != want).sum())} entries wrong: flagged tokens must equal the exact encoder's, all others stay"
    # count = 0 is a no-op
    before = codes.clone()
    _fix(vq, audio, ids, 0, halo, win, codes)
    assert torch.equal(codes, before)
    # a window of the whole clip
    codes.fill_(-1)
    two = [3, t + t - 2]
    _fix(vq, audio, two, 2, halo, t, codes)
    want.fill_(-1)
    want[two] = ref.flatten().cpu()[two]
    assert torch.equal(codes.flatten().cpu(), want)
    # a window that cannot hold a token's halo on both sides
    with pytest.raises(_lib.LlarkHipError, match="shorter"):
        _fix(vq, audio, two, 2, halo, 2 * halo, codes)
    assert torch.equal(codes.flatten().cpu(), want)
