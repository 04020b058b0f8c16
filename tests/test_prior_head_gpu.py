"""GPU: the one-pass head of the prior (llark_prior_head) against the three kernels it replaces -- llark_prior_embed,
llark_layernorm_split_f16 and llark_ln_row_pred -- and the 16-byte-load form of llark_ln_stats_finalize(_p) against the one-load-per-slice
loop it keeps for unaligned operands.  Everything here is bit-equality: the fused kernels reorder memory traffic, never arithmetic."""
import pytest
import torch

from llark_amd.jukebox.hparams import hparams_5b_depth
from llark_amd.jukebox.synthetic import make_prior_weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_pred", [True, False])
@pytest.mark.parametrize("n,t,width", [(2, 16, 4800), (2, 16, 192), (1, 7, 192)])         # 5b width, the tiny twin's, a last workgroup with 3 of 4 rows
def test_prior_head_equals_the_three_kernels(n, t, width, with_pred):
    from llark_amd import ops
    gen = torch.Generator().manual_seed(width + t)
    bins, rows, ldo = 64, n * t, ops.round_up(width, 32)
    z = torch.randint(0, bins, (n, t), generator=gen)
    z[0, 1], z[-1, 2] = -3, bins + 5                                    # out-of-range codes are clamped the same way
    z = z.cuda()
    x_emb, pos_emb, x_cond = ((torch.randn(r, width, generator=gen) * s).cuda() for r, s in ((bins, 0.02), (t, 0.01), (t, 3.0)))
    y_cond = torch.randn(width, generator=gen).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(width, generator=gen)).cuda(), (0.1 * torch.randn(width, generator=gen)).cuda()

    def planes():
        return torch.zeros(rows, ldo, dtype=torch.float16, device="cuda"), torch.zeros(rows, ldo, dtype=torch.float16, device="cuda")

    h_ref = ops.prior_embed(z, x_emb, pos_emb, x_cond, y_cond)
    hi_ref, lo_ref = planes()
    ops.layernorm_split(h_ref.view(rows, width), gamma, beta, 1e-5, hi_ref, lo_ref)
    pred_ref = torch.zeros(rows, 2, device="cuda")
    ops.ln_row_pred(h_ref.view(rows, width), 1e-5, pred_ref)

    assert ops.prior_head_takes(width, ldo)
    hi, lo = planes()
    pred = torch.zeros(rows, 2, device="cuda") if with_pred else None
    h = ops.prior_head(z, x_emb, pos_emb, x_cond, y_cond, gamma, beta, 1e-5, hi, lo, pred)
    assert torch.equal(h, h_ref), "h differs from prior_embed"
    assert torch.equal(hi, hi_ref) and torch.equal(lo, lo_ref), "the ln_0 planes differ from layernorm_split"
    assert (lo_ref[:, :width] != 0).any()
    if with_pred:
        assert torch.equal(pred, pred_ref), "pred differs from ln_row_pred"


@pytest.mark.parametrize("with_pred", [True, False])
@pytest.mark.parametrize("nparts", [38, 6, 22])                          # 5b width (two batches of loads), one partial batch, one batch + 1
def test_ln_stats_finalize_equals_the_per_slice_loop(nparts, with_pred):
    from llark_amd import ops
    gen = torch.Generator().manual_seed(nparts)
    rows, width = 1000, nparts * 128                                     # 4 workgroups, the last one partly empty
    x = torch.randn(rows, nparts, 128, generator=gen) * (0.5 + torch.rand(rows, 1, 1, generator=gen)) + torch.randn(rows, 1, 1, generator=gen)
    part = torch.stack((x.sum(dim=2), (x * x).sum(dim=2)), dim=2).contiguous().cuda()
    # the same values 8 bytes off a 16-byte boundary: the entry point then runs the loop with one 8-byte load per slice
    buf = torch.empty(part.numel() + 2, device="cuda")
    part_off = buf[2:]
    part_off.copy_(part.flatten())
    assert part.data_ptr() % 16 == 0 and part_off.data_ptr() % 16 == 8
    pred0 = torch.stack((torch.randn(rows, generator=gen), torch.exp2(torch.randint(-3, 4, (rows,), generator=gen).float())), dim=1).cuda()
    out = []
    for p in (part, part_off.view(rows, nparts, 2)):
        stat = torch.zeros(rows, 2, device="cuda")
        pred = pred0.clone() if with_pred else None
        ops.ln_stats_finalize(p, rows, nparts, width, 1e-5, stat, pred)
        out.append((stat, pred))
    assert torch.isfinite(out[0][0]).all() and (out[0][0][:, 1] > 0).all()
    assert torch.equal(out[0][0], out[1][0]), "stat differs between the 16-byte-load form and the per-slice loop"
    if with_pred:
        assert torch.equal(out[0][1], out[1][1]) and not torch.equal(out[0][1], pred0), "the replaced pred differs"


def test_forward_with_the_fused_head_is_bit_equal(monkeypatch):
    """PriorTransformer.forward on the folded path (5b widths, one clip, one layer): the one-pass head against LLARK_PRIOR_FUSED_HEAD=0."""
    from llark_amd import ops
    from llark_amd.jukebox import extract as E
    from llark_amd.jukebox.prior import TopPrior
    hps = hparams_5b_depth(1)
    w = make_prior_weights(hps, 7, depth=1)
    z = torch.randint(0, hps.l_bins, (1, hps.n_ctx), generator=torch.Generator().manual_seed(8)).cuda()
    tp_new = TopPrior(hps, w, "cuda", depth=1)
    monkeypatch.setenv("LLARK_PRIOR_FUSED_HEAD", "0")
    tp_old = TopPrior(hps, w, "cuda", depth=1)
    assert tp_new.prior.fused_head and not tp_old.prior.fused_head
    x_cond, y_cond = E.get_cond(hps, tp_new)
    calls = []
    real = ops.prior_head
    monkeypatch.setattr(ops, "prior_head", lambda *a, **k: calls.append(1) or real(*a, **k))
    a_new = E.get_final_activations(z, x_cond, y_cond, tp_new)
    assert calls == [1] and tp_new.prior._fold_rows, "the one-pass head was not taken on the folded path"
    a_old = E.get_final_activations(z, x_cond, y_cond, tp_old)
    assert calls == [1]
    assert torch.equal(a_new, a_old)
