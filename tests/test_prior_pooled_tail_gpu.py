"""GPU: the pooled tail of the prior -- the windowed mean taken BEFORE the last block's second MLP product
(llark_pool_window_tail + one product of `frames` rows per clip) against the full-M product followed by llark_pool_window.

Kernel level: the h half is bit-equal to llark_pool_window; the pooled planes are the window mean of float(hi) + float(lo) to
(frame_len + 2) 2^-24 max|g| -- the fp32 sequential sum (frame_len - 1 additions of partial sums <= frame_len max|g|, then the division
by frame_len: each rounds at 2^-24 relative) plus 2 2^-24 |x| for the hi / lo split; pad columns exactly 0; windows never cross a clip.
Path level: both paths against a float64 evaluation of the last block from the SAME h_mid and g planes; the pooled path's max-abs error
must stay within 2x the full path's (one extra hi / lo split)."""
import pytest
import torch

from llark_amd.jukebox.hparams import hparams_5b_depth, hparams_tiny
from llark_amd.jukebox.synthetic import make_prior_weights

pytestmark = pytest.mark.gpu

N, T, W, LD = 2, 70, 72, 96


def _planes(g, ld, pad_value=0.0):
    """fp32 [rows][w] -> fp16 hi / lo planes [rows][ld] with a nonzero lo; the pad columns hold `pad_value`."""
    rows, w = g.shape
    hi = torch.full((rows, ld), pad_value, dtype=torch.float16, device=g.device)
    lo = torch.full((rows, ld), pad_value, dtype=torch.float16, device=g.device)
    hi[:, :w] = g.half()
    lo[:, :w] = (g - hi[:, :w].float()).half()
    assert (lo[:, :w] != 0).any()
    return hi, lo


@pytest.mark.parametrize("frame_len", [34, 1, 70])
def test_pool_window_tail_kernel(frame_len):
    from llark_amd import ops
    gen = torch.Generator().manual_seed(frame_len)
    frames = T // frame_len                                        # 34 -> 2 frames, 2 rows of every clip dropped
    h = (torch.randn(N, T, W, generator=gen) * 3).cuda()
    g = (torch.randn(N * T, W, generator=gen) * 2).cuda()
    g_hi, g_lo = _planes(g, LD, pad_value=1.0)                     # garbage in the pad columns of the input: the output's must be 0 anyway
    pool_h, pg_hi, pg_lo = ops.pool_window_tail(h, g_hi, g_lo, W, frame_len, frames)
    assert pool_h.shape == (N * frames, W) and pg_hi.shape == pg_lo.shape == (N * frames, LD)
    assert torch.equal(pool_h.view(N, frames, W), ops.pool_window(h, frame_len, frames)), "the h half is not bit-equal to pool_window"
    g64 = (g_hi.double() + g_lo.double())[:, :W].view(N, T, W)[:, : frames * frame_len].reshape(N, frames, frame_len, W)
    ref = g64.mean(dim=2).reshape(N * frames, W)
    got = (pg_hi.double() + pg_lo.double())[:, :W]
    err, bound = float((got - ref).abs().max()), (frame_len + 2) * 2.0 ** -24 * float(g64.abs().max())
    print(f"\n[pool-tail] frame_len {frame_len}: pooled planes max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert (pg_hi[:, W:] == 0).all() and (pg_lo[:, W:] == 0).all(), "pad columns of the pooled planes are not zero"


def test_pool_window_tail_never_crosses_a_clip():
    from llark_amd import ops
    h = torch.zeros(N, T, W, device="cuda")
    h[1] = 1.0
    g = torch.zeros(N * T, W, device="cuda")
    g[T:] = 1.0
    g_hi = torch.zeros(N * T, LD, dtype=torch.float16, device="cuda")
    g_lo = torch.zeros_like(g_hi)
    g_hi[:, :W] = g.half()
    for frame_len in (34, 1, 70):
        frames = T // frame_len
        pool_h, pg_hi, pg_lo = ops.pool_window_tail(h, g_hi, g_lo, W, frame_len, frames)
        for clip, want in ((0, 0.0), (1, 1.0)):
            rows = slice(clip * frames, (clip + 1) * frames)
            assert (pool_h[rows] == want).all(), f"frame_len {frame_len}: clip {clip} of pool_h mixes clips"
            assert (pg_hi[rows, :W] == want).all() and (pg_lo[rows] == 0).all(), f"frame_len {frame_len}: clip {clip} of the planes mixes clips"


def _both_paths_against_float64(monkeypatch, tp, z, frame_len):
    """(pooled path, full path followed by pool_window, float64 evaluation of the last block from the h_mid and g planes the pooled
    path itself pooled)."""
    from llark_amd import ops
    from llark_amd.jukebox import extract as E
    pr, hps = tp.prior, tp.hps
    x_cond, y_cond = E.get_cond(hps, tp)
    pr.only_encode = True
    frames = hps.n_ctx // frame_len
    seen = {}
    real = ops.pool_window_tail

    def spy(h, g_hi, g_lo, gwidth, fl, fr):
        seen.update(h=h.clone(), g_hi=g_hi.clone(), g_lo=g_lo.clone(), gwidth=gwidth)
        return real(h, g_hi, g_lo, gwidth, fl, fr)

    monkeypatch.setattr(ops, "pool_window_tail", spy)
    pooled = pr.forward(z.cuda(), x_cond=x_cond, y_cond=y_cond, pool=(frame_len, frames))
    monkeypatch.setattr(ops, "pool_window_tail", real)
    assert seen, "forward(pool=) did not take the pooled tail"
    full = ops.pool_window(pr.forward(z.cuda(), x_cond=x_cond, y_cond=y_cond), frame_len, frames)
    L = pr.layers[pr.depth - 1]
    K = seen["gwidth"]
    g64 = (seen["g_hi"].double() + seen["g_lo"].double())[:, :K]
    out64 = seen["h"].double().view(-1, pr.width) + g64 @ L.w_proj2[:, :K].double().t() + L.b_proj2.double()
    n = z.shape[0]
    ref = out64.view(n, hps.n_ctx, pr.width)[:, : frames * frame_len].reshape(n, frames, frame_len, pr.width).mean(dim=2)
    return pooled, full, ref


@pytest.mark.parametrize("frame_len", [34, 1])
def test_pooled_tail_path_tiny(monkeypatch, frame_len):
    """hparams_tiny, B = 2: error of forward(pool=) and of pool_window(forward()) against float64, window by window (frame_len 34) and
    row by row (frame_len 1)."""
    from llark_amd.jukebox.prior import TopPrior
    hps = hparams_tiny()
    tp = TopPrior(hps, make_prior_weights(hps, 3, depth=3), "cuda", depth=3)
    z = torch.randint(0, hps.l_bins, (2, hps.n_ctx), generator=torch.Generator().manual_seed(5))
    assert tp.prior.pooled_tail
    pooled, full, ref = _both_paths_against_float64(monkeypatch, tp, z, frame_len)
    assert pooled.shape == full.shape == ref.shape == (2, hps.n_ctx // frame_len, hps.prior_width)
    e_pooled, e_full = float((pooled.double() - ref).abs().max()), float((full.double() - ref).abs().max())
    print(f"\n[pool-tail] tiny twin, frame_len {frame_len}: pooled path max err {e_pooled:.3e}, full path {e_full:.3e}, max|ref| {float(ref.abs().max()):.3f}")
    assert e_pooled <= 2.0 * e_full


def test_pooled_tail_path_folded_5b_width(monkeypatch):
    """The folded-LayerNorm path (5b widths, one clip, one layer), where the last block is _layer_forward_fold.  At K = 4800 the two
    paths do not share an error model: the full path's fp32 accumulation errors are averaged over the window's 34 rows, the pooled
    product's single accumulation is not, so its error is not held to a multiple of the full path's here (measured on MI355X: pooled
    1.68e-6, full 4.94e-7, max|ref| 1.74).  Each path is held to the bound the per-block outputs of this prior are held to against the
    oracle (tests/test_prior_gpu.py: 2e-5 of max|ref|), against the float64 evaluation from the same h_mid and g planes."""
    from llark_amd.jukebox.prior import TopPrior
    hps = hparams_5b_depth(1)
    tp = TopPrior(hps, make_prior_weights(hps, 4, depth=1), "cuda", depth=1)
    z = torch.randint(0, hps.l_bins, (1, hps.n_ctx), generator=torch.Generator().manual_seed(6))
    pooled, full, ref = _both_paths_against_float64(monkeypatch, tp, z, 34)
    assert tp.prior._fold_rows, "the folded path was not taken at 8192 rows"
    e_pooled, e_full, scale = float((pooled.double() - ref).abs().max()), float((full.double() - ref).abs().max()), float(ref.abs().max())
    print(f"\n[pool-tail] 5b widths, folded: pooled path max err {e_pooled:.3e}, full path {e_full:.3e}, max|ref| {scale:.3f}")
    assert e_pooled <= 2e-5 * scale and e_full <= 2e-5 * scale


def test_pooled_tail_clip_does_not_depend_on_its_batch():
    """The pooled product runs per clip (m = frames, whatever the batch): clip 0 of a batch of 3 is bit-equal to clip 0 alone, at the
    tiny twin's 15 frames (the weight-streaming kernel, one launch per clip) and at 512 (the tile kernel, clips in one launch)."""
    from llark_amd.jukebox import extract as E
    from llark_amd.jukebox.prior import TopPrior
    hps = hparams_tiny()
    tp = TopPrior(hps, make_prior_weights(hps, 3, depth=3), "cuda", depth=3)
    tp.prior.only_encode = True
    x_cond, y_cond = E.get_cond(hps, tp)
    z = torch.randint(0, hps.l_bins, (3, hps.n_ctx), generator=torch.Generator().manual_seed(9)).cuda()
    for frame_len in (34, 1):
        pool = (frame_len, hps.n_ctx // frame_len)
        alone = tp.prior.forward(z[:1], x_cond=x_cond, y_cond=y_cond, pool=pool)
        batch = tp.prior.forward(z, x_cond=x_cond, y_cond=y_cond, pool=pool)
        assert torch.equal(batch[0], alone[0]), f"frame_len {frame_len}: clip 0 of a batch differs from clip 0 alone"


def test_pooled_tail_knob_off_is_the_full_sequence(monkeypatch):
    """LLARK_PRIOR_POOLED_TAIL=0: forward(pool=) is the full product followed by pool_window, bit for bit."""
    from llark_amd import ops
    from llark_amd.jukebox import extract as E
    from llark_amd.jukebox.prior import TopPrior
    hps = hparams_tiny()
    w = make_prior_weights(hps, 3, depth=3)
    monkeypatch.setenv("LLARK_PRIOR_POOLED_TAIL", "0")
    tp = TopPrior(hps, w, "cuda", depth=3)
    assert not tp.prior.pooled_tail
    tp.prior.only_encode = True
    x_cond, y_cond = E.get_cond(hps, tp)
    z = torch.randint(0, hps.l_bins, (2, hps.n_ctx), generator=torch.Generator().manual_seed(5)).cuda()
    monkeypatch.setattr(ops, "pool_window_tail", lambda *a, **k: pytest.fail("the pooled tail ran with the knob off"))
    got = tp.prior.forward(z, x_cond=x_cond, y_cond=y_cond, pool=(34, hps.n_ctx // 34))
    assert torch.equal(got, ops.pool_window(tp.prior.forward(z, x_cond=x_cond, y_cond=y_cond), 34, hps.n_ctx // 34))
