"""The LoRA kernels of csrc/lora.hip, one at a time, against float64 products of the bf16-rounded inputs (the convention of
tests/test_train_kernels_gpu.py; errors are measured against max|ref|).

Bars: fp32 outputs <= 1e-5 max|ref| (the RMSNorm-backward bar); llark_lora_down's bf16 output <= 2**-7 max|ref| (one bf16
rounding).  llark_lora_dw joins its token-split partial sums in a second launch in a fixed order: no atomics on the gradient, so
two runs are compared bit for bit; only ``sumsq`` is an atomic sum of doubles (rtol = atol = 1e-4 like the per-workgroup partials
of the existing tests is far above what a double sum can lose; 1e-9 relative is asserted).
Memory around every output is pre-filled with a sentinel and asserted bit-unchanged."""
import pytest
import torch

from kernel_util import assert_untouched, bf_sentinel, bits, gen

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _bf(shape, *key, std=1.0):
    return (torch.randn(shape, generator=gen(*key)) * std).to(BF)


@pytest.mark.parametrize("rows,K,rp_total", [(r, k, p) for r in (40, 144, 261) for k in (256, 512) for p in (64, 192)]
                         + [(40, 272, 64), (33, 784, 128)]                 # + k that is no multiple of the 256-wide staged chunk
                         + [(144, 2048, 64), (261, 1024, 128), (1040, 1024, 64)])   # + the contraction split over 4 / 2 / 2 workgroups per tile
def test_lora_down_into_the_tail_of_a_wider_buffer(rows, K, rp_total):
    """out = x . m^T lands in columns [K, K + rp_total) of a [rows][K + rp_total + 8] buffer whose other columns (x itself in the
    first K: the augmented-activation layout) stay bit-unchanged.  Catches a wrong k step of a wave, a wrong accumulator-to-row
    map, a missing row mask (rows % 32 != 0) and a wrong column block (rp_total = 192: three column blocks)."""
    from llark_amd import ops
    ld = K + rp_total + 8
    buf = bf_sentinel((rows, ld))
    buf[:, :K] = _bf((rows, K), 1, rows, K)
    m = _bf((rp_total, K), 2, rp_total, K, std=K ** -0.5)
    ref = buf[:, :K].double() @ m.double().t()
    d = buf.cuda()
    from llark_amd import _lib
    assert (_lib.lib().llark_lora_down_scratch_bytes(rows, K, rp_total) > 0) == (K >= 1024)
    ops.lora_down(d[:, :K], m.cuda(), d[:, K: K + rp_total])
    torch.cuda.synchronize()
    got = d.cpu()
    written = torch.zeros((rows, ld), dtype=torch.bool)
    written[:, K: K + rp_total] = True
    assert_untouched("lora_down", got, buf, written)
    err = (got[:, K: K + rp_total].double() - ref).abs().max().item()
    print(f"lora_down rows={rows} K={K} rp={rp_total}: err {err:.3e}, max|ref| {ref.abs().max().item():.3e}")
    assert err <= 2.0 ** -7 * ref.abs().max().item()


@pytest.mark.parametrize("toks", [40, 144, 261])
@pytest.mark.parametrize("big", [256, 768])
@pytest.mark.parametrize("r", [8, 64])
@pytest.mark.parametrize("accumulate", [False, True])
def test_lora_dw_window_accumulate_sumsq(toks, big, r, accumulate):
    """g (= | +=) scale P^T Q with P a column window of a wider matrix and Q a column window of a stacked T; the rank padding
    (columns r .. 63) takes nothing; sumsq = the float64 sum of squares of what was stored.  Catches a wrong token mask at a split's
    end (toks % 64 != 0), a wrong split stride, a dropped scale, accumulate ignored, and padding that receives a gradient."""
    from llark_amd import ops
    rp, c0, q0 = 64, 32, 64
    P = _bf((toks, big + 96), 3, toks, big)
    Q = _bf((toks, 3 * rp), 4, toks, r)                        # NOT zero in the padded columns: the kernel itself must mask them
    g0 = torch.randn((big, rp), generator=gen(5, big, r))
    scale = 0.25
    ref = scale * (P[:, c0: c0 + big].double().t() @ Q[:, q0: q0 + rp].double())
    ref[:, r:] = 0.0
    if accumulate:
        ref = ref + g0.double()
    flat = torch.full((3 * 4 + big * rp + 8,), float("nan"))
    flat[12: 12 + big * rp] = g0.reshape(-1)
    before = flat.clone()
    d = flat.cuda()
    g = d[12: 12 + big * rp].view(big, rp)
    ss = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
    Pd, Qd = P.cuda(), Q.cuda()
    ops.lora_dw(Pd[:, c0:], Qd[:, q0: q0 + rp], g, r, scale, accumulate=accumulate, sumsq=ss)
    torch.cuda.synchronize()
    got = d.cpu()
    written = torch.zeros_like(flat, dtype=torch.bool)
    written[12: 12 + big * rp] = True
    assert_untouched("lora_dw", got, before, written)
    assert torch.equal(bits(Pd), bits(P)) and torch.equal(bits(Qd), bits(Q))
    gg = got[12: 12 + big * rp].view(big, rp)
    err = (gg.double() - ref).abs().max().item()
    print(f"lora_dw toks={toks} big={big} r={r} acc={accumulate}: err {err:.3e}, max|ref| {ref.abs().max().item():.3e}")
    assert err <= 1e-5 * ref.abs().max().item()
    if not accumulate:
        assert gg[:, r:].abs().max().item() == 0.0 if r < rp else True
    want_ss = 3.0 + float((gg.double() ** 2).sum())
    assert abs(ss.item() - want_ss) <= 1e-9 * want_ss
    # a second run gives the same bits: the partial sums meet in a fixed order
    g2 = g0.cuda().clone()
    g3 = g0.cuda().clone()
    ops.lora_dw(Pd[:, c0:], Qd[:, q0: q0 + rp], g2, r, scale, accumulate=accumulate)
    ops.lora_dw(Pd[:, c0:], Qd[:, q0: q0 + rp], g3, r, scale, accumulate=accumulate)
    assert torch.equal(g2, g3) and torch.equal(g2.cpu(), gg)


def test_lora_dw_interleaved_column_blocks():
    """p_blk = 64: logical column i of P is physical column (i // 32) * 64 + i % 32 (+ 32 for the `up` half): the gate and up
    gradients of the interleaved gate|up layout."""
    from llark_amd import ops
    toks, I, rp = 144, 256, 64
    dgu = _bf((toks, 2 * I), 6)
    T = _bf((toks, 2 * rp), 7)
    v = dgu.view(toks, I // 32, 2, 32)
    for half in (0, 1):
        ref = v[:, :, half].reshape(toks, I).double().t() @ T[:, half * rp: (half + 1) * rp].double()
        g = torch.empty((I, rp), device="cuda")
        ops.lora_dw(dgu.cuda()[:, 32 * half:], T.cuda()[:, half * rp: (half + 1) * rp], g, 64, 1.0, p_blk=64)
        assert (g.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("blk,row0", [(32, 0), (32, 64), (64, 0), (64, 32)])
def test_lora_refresh_writes_only_its_own_blocks(blk, row0):
    """dst / dst_t are blocks of wider operands: exactly bf16(scale * src) at rows row0 + row_of(i), its transpose in dst_t, and not one
    other element touched.  Catches a wrong row map (interleaved gate / up rows) and a transposed tile written to the wrong side."""
    from llark_amd import ops
    rows, rp, s = 96, 64, 0.25
    src = torch.randn((rows, rp), generator=gen(8, blk, row0))
    src[:, 8:] = 0.0
    ngrp = row0 + (rows // 32) * blk + 32
    diag = bf_sentinel((ngrp, 3 * rp))
    tr = bf_sentinel((3 * rp, ngrp))
    dd, dt = diag.cuda(), tr.cuda()
    ops.lora_refresh(src.cuda(), s, dd[row0:, rp: 2 * rp], dt[rp: 2 * rp, row0:], blk)
    torch.cuda.synchronize()
    rmap = torch.tensor([row0 + (i // 32) * blk + i % 32 for i in range(rows)])
    want = (src * s).to(BF)
    wd, wt = diag.clone(), tr.clone()
    wd[rmap, rp: 2 * rp] = want
    wt[rp: 2 * rp, rmap] = want.t()
    assert torch.equal(bits(dd), bits(wd))
    assert torch.equal(bits(dt), bits(wt))


def test_unsupported_shapes_are_declined_before_any_launch():
    from llark_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros((64, 256), dtype=BF, device="cuda")
    m = torch.zeros((64, 256), dtype=BF, device="cuda")
    out = bf_sentinel((64, 64)).cuda()
    before = out.clone()
    s = torch.cuda.current_stream().cuda_stream
    U = ops.ERR_UNSUPPORTED
    assert L.llark_lora_down(x.data_ptr(), 256, m.data_ptr(), 256, 64, 250, 64, out.data_ptr(), 64, None, 0, s) == U     # k % 16
    assert L.llark_lora_down(x.data_ptr(), 256, m.data_ptr(), 256, 64, 256, 48, out.data_ptr(), 64, None, 0, s) == U     # rp_total % 64
    assert L.llark_lora_down(x.data_ptr(), 252, m.data_ptr(), 256, 64, 128, 64, out.data_ptr(), 64, None, 0, s) == U     # lda % 8
    assert L.llark_lora_down(x.data_ptr() + 2, 256, m.data_ptr(), 256, 63, 128, 64, out.data_ptr(), 64, None, 0, s) == U  # alignment
    g = torch.zeros((256, 64), device="cuda")
    scr = torch.zeros((1 << 20,), device="cuda")
    args = lambda big, rp, r, pblk, nbytes: (x.data_ptr(), 256, pblk, m.data_ptr(), 256, 64, big, rp, r, 1.0, g.data_ptr(), 0, None,
                                             scr.data_ptr(), nbytes, s)
    assert L.llark_lora_dw(*args(250, 64, 8, 32, 1 << 22)) == U          # big % 32
    assert L.llark_lora_dw(*args(256, 96, 8, 32, 1 << 22)) == U          # rp % 64
    assert L.llark_lora_dw(*args(256, 64, 72, 32, 1 << 22)) == U         # r > rp
    assert L.llark_lora_dw(*args(256, 64, 8, 48, 1 << 22)) == U          # p_blk % 32
    assert L.llark_lora_dw(*args(256, 64, 8, 32, 16)) == U               # scratch too small
    assert L.llark_lora_dw_scratch_bytes(64, 250, 64) == 0
    src = torch.zeros((64, 64), device="cuda")
    assert L.llark_lora_refresh(src.data_ptr(), 60, 64, 1.0, 32, out.data_ptr(), 64, None, 0, s) == U           # rows % 32
    assert L.llark_lora_refresh(src.data_ptr(), 64, 64, 1.0, 32, out.data_ptr(), 32, None, 0, s) == U           # ld_dst < rp
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(before)) and g.abs().max().item() == 0.0
