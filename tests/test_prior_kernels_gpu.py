"""GPU: the kernels of csrc/prior.hip, one at a time through llark_amd.ops, against the float64 references and bounds of
tests/prior_kernel_ref.py (see its docstring for the bounds, their derivation and the measured ratios; tests/test_prior_kernel_ref_cpu.py
shows that those bounds reject wrong kernels).  Every output lives in a sentinel-filled buffer with pad columns, every input pad holds
NaN: whatever a kernel writes outside its output, or reads outside its input, shows.

1. factored attention (prior_attn16_kernel<1 .. 5>), fp16 and lo8 low planes, the launcher's refusals
2. LayerNorm -> planes (layernorm_split8_kernel<1 | 4 | 10 | 16>, layernorm_split_kernel<1 | 4 | 16 | 19 | 32>), fp16 and lo8
3. prior_head_kernel<1 | 4 | 16> bit-equal to the three kernels it fuses; prior_embed bit-equal to torch; ln_row_pred
4. pool_window, pool_mean, zero_pad16
"""
import pytest
import torch

import prior_kernel_ref as R
from kernel_util import assert_untouched, bits, f16_sentinel, gen, mask, nan_buf, tol, u8_sentinel

pytestmark = pytest.mark.gpu


def _sync():
    torch.cuda.synchronize()


# =====================================================================================================================
# 1. factored attention
# =====================================================================================================================
def _run_attn(ref, lo8=False):
    from llark_amd import ops
    i = ref.inp
    S, rows = i.heads * i.hd, i.n * i.t
    ldq, ldo = 3 * S + 6, S + 2
    qkv = R.qkv_rows(i, ldq)
    hi0 = f16_sentinel((rows, ldo))
    lo0 = u8_sentinel((rows, R.round_up(S, 64) + 64)) if lo8 else f16_sentinel((rows, ldo))
    qg, hi, lo = qkv.cuda(), hi0.cuda(), lo0.cuda()
    ops.prior_attn(qg, i.n, i.t, S, i.heads, i.blocks, i.pattern, hi, lo)
    _sync()
    assert torch.equal(bits(qg), bits(qkv)), "qkv was modified"
    assert_untouched("hi plane", hi, hi0, mask(hi0.shape, rows, 0, S))
    assert_untouched("lo plane", lo, lo0, R.lo8_written(rows, lo0.shape[1], S) if lo8 else mask(lo0.shape, rows, 0, S))
    return hi.cpu(), lo.cpu(), S


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case,scale", R.ATTN_RUNS, ids=lambda v: str(v))
def test_prior_attn_matches_float64(case, scale, pattern):
    ref = R.attn_reference(case, pattern, scale)
    i = ref.inp
    hi, lo, S = _run_attn(ref)
    got = hi[:, :S].double() + lo[:, :S].double()
    assert bool(torch.isfinite(got).all())
    R.check_attn(f"prior_attn {case} {scale} pattern {pattern}", R.from_rows(got, i.n, i.heads), ref)
    if pattern == 3:                                     # block 0 sees nothing: exact +0 in both planes
        blk0 = R.to_rows(torch.arange(i.t)[None, None, :, None].expand(i.n, i.heads, i.t, i.hd) < i.bc)
        assert not bool(bits(hi[:, :S])[blk0].any()) and not bool(bits(lo[:, :S])[blk0].any())


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", R.LO8_CASES)
def test_prior_attn_lo8_matches_float64(case, pattern):
    from llark_amd import ops
    ref = R.attn_reference(case, pattern)
    i = ref.inp
    hi, lo8, S = _run_attn(ref, lo8=True)
    hi64 = hi[:, :S].double()
    got = hi64 + ops.lo8_decode(lo8, S).double()
    assert bool(torch.isfinite(got).all())
    extra = R.e4m3_term(R.to_rows(ref.out), hi64, ops.LO8_SA)
    R.check_attn(f"prior_attn_lo8 {case} pattern {pattern}", R.from_rows(got, i.n, i.heads), ref,
                 extra=R.from_rows(torch.from_numpy(extra), i.n, i.heads).numpy())
    if pattern == 3:
        blk0 = torch.arange(i.n * i.t) % i.t < i.bc
        assert not bool(bits(hi[:, :S])[blk0].any())
        assert not bool(lo8[blk0][:, R.lo8_pos(torch.arange(S))].any()), "block 0 of the previous-block pattern must write byte 0x00"


@pytest.mark.parametrize("name", list(R.ATTN_REFUSALS))
def test_prior_attn_refusals_launch_nothing(name):
    from llark_amd import _lib
    t, S, heads, blocks, pattern, ldq, ldo = R.ATTN_REFUSALS[name]
    # buffers large enough for the call had it been taken
    qkv = torch.zeros((t, max(ldq, 3 * S) + 8), device="cuda")
    hi0 = f16_sentinel((t, max(ldo, S) + 8))
    hi, lo = hi0.cuda(), hi0.cuda()
    _sync()
    rc = _lib.lib().llark_prior_attn(qkv.data_ptr(), ldq, 1, t, S, heads, blocks, pattern, hi.data_ptr(), lo.data_ptr(), ldo,
                                     torch.cuda.current_stream().cuda_stream)
    _sync()
    assert rc != 0, f"{name}: accepted"
    nothing = torch.zeros(hi0.shape, dtype=torch.bool)
    assert_untouched(f"{name}: hi", hi, hi0, nothing)
    assert_untouched(f"{name}: lo", lo, hi0, nothing)


# =====================================================================================================================
# 2. LayerNorm -> planes
# =====================================================================================================================
def _ln_case(width, forced4, lo8):
    from llark_amd import ops
    ldx, ldo = R.ln_lds(width, forced4)
    assert R.ln_rule(width, ldx, ldo)[0] == ("8" if width % 8 == 0 and not forced4 else "4")
    for rows in R.LN_ROWS:
        for data in R.LN_DATA:
            x, gamma, beta = R.ln_inputs(rows, width, data)
            ref, atol, r = R.ln_reference(x, gamma, beta)
            xb = nan_buf(rows, ldx)
            xb[:, :width] = x
            hi0 = f16_sentinel((rows, ldo))
            lo0 = u8_sentinel((rows, R.round_up(width, 64) + 64)) if lo8 else f16_sentinel((rows, ldo))
            xg, hi, lo = xb.cuda(), hi0.cuda(), lo0.cuda()
            name = f"layernorm_split{'_lo8' if lo8 else ''}[{rows}x{width} ldx {ldx} ldo {ldo} {data}]"
            if lo8:
                ops.layernorm_split_lo8(xg[:, :width], gamma.cuda(), beta.cuda(), R.LN_EPS, hi, lo)
            else:
                ops.layernorm_split(xg[:, :width], gamma.cuda(), beta.cuda(), R.LN_EPS, hi, lo)
            _sync()
            assert torch.equal(bits(xg), bits(xb)), f"{name}: x was modified"
            assert_untouched(f"{name} hi", hi, hi0, mask(hi0.shape, rows, 0, width))
            assert_untouched(f"{name} lo", lo, lo0, R.lo8_written(rows, lo0.shape[1], width) if lo8 else mask(lo0.shape, rows, 0, width))
            hi64 = hi.cpu()[:, :width].double()
            if lo8:
                got = hi64 + ops.lo8_decode(lo.cpu(), width).double()
                atol = atol + R.e4m3_term(ref, hi64, ops.LO8_SA)
            else:
                got = hi64 + lo.cpu()[:, :width].double()
            R.check_frac(name, got, ref, atol, r)


@pytest.mark.parametrize("width", R.LN8_WIDTHS + R.LN4_WIDTHS)
def test_layernorm_split_matches_float64(width):
    _ln_case(width, False, False)


@pytest.mark.parametrize("width", R.LN_FORCED4)
def test_layernorm_split_four_column_form_at_a_multiple_of_8(width):
    _ln_case(width, True, False)


@pytest.mark.parametrize("width", R.LN_LO8_WIDTHS)
def test_layernorm_split_lo8_matches_float64(width):
    _ln_case(width, False, True)


@pytest.mark.parametrize("lo8", [False, True], ids=["f16", "lo8"])
@pytest.mark.parametrize("width", [8200, 8196])
def test_layernorm_split_refuses_widths_over_8192(width, lo8):
    from llark_amd import _lib, ops
    assert R.ln_rule(width, width, width) is None
    x = torch.zeros((4, width), device="cuda")
    ones = torch.ones(width, device="cuda")
    hi0 = f16_sentinel((4, width))
    lo0 = u8_sentinel((4, R.round_up(width, 64))) if lo8 else hi0
    hi, lo = hi0.cuda(), lo0.cuda()
    with pytest.raises(_lib.LlarkHipError, match="too large"):
        (ops.layernorm_split_lo8 if lo8 else ops.layernorm_split)(x, ones, ones, R.LN_EPS, hi, lo)
    _sync()
    assert_untouched("hi", hi, hi0, torch.zeros(hi0.shape, dtype=torch.bool))
    assert_untouched("lo", lo, lo0, torch.zeros(lo0.shape, dtype=torch.bool))


# =====================================================================================================================
# 3. the head of a forward: prior_embed, prior_head, ln_row_pred
# =====================================================================================================================
def _embed_inputs(n, t, width, bins, seed):
    g = gen(n, t, width, seed)
    z = torch.randint(0, bins, (n, t), generator=g)
    z[0, 1], z[-1, 0] = -3, bins + 2                       # out-of-range codes clamp to the first / last row of the table
    x_emb = torch.randn(bins, width, generator=g) * 0.5
    pos_emb = torch.randn(t, width, generator=g) * 0.1
    x_cond = torch.randn(t, width, generator=g) * 3.0
    y_cond = torch.randn(width, generator=g)
    return z, x_emb, pos_emb, x_cond, y_cond


def _embed_torch(z, x_emb, pos_emb, x_cond, y_cond):
    """fp32 on the CPU, the kernel's association: ((x_emb[z[t - 1]] | y_cond) + pos_emb) + x_cond"""
    n, t = z.shape
    e = x_emb[z.clamp(0, x_emb.shape[0] - 1)]
    e = torch.cat((y_cond.expand(n, 1, -1), e[:, :-1]), dim=1)
    return (e + pos_emb) + x_cond


@pytest.mark.parametrize("n,t,width", [(2, 3, 8), (3, 5, 260), (2, 600, 3600)], ids=lambda v: str(v))
def test_prior_embed_is_bit_equal_to_torch(n, t, width):
    """(2, 600, 3600) = 1 080 000 float4 items: more than the 4096 x 256 threads of the capped grid, so the grid-stride loop runs"""
    from llark_amd import ops
    bins = 7
    z, x_emb, pos_emb, x_cond, y_cond = _embed_inputs(n, t, width, bins, 1)
    assert (n * t * width // 4 > 4096 * 256) == (t == 600)
    ref = _embed_torch(z, x_emb, pos_emb, x_cond, y_cond)
    dev = [a.cuda() for a in (x_emb, pos_emb, x_cond, y_cond)]
    got = ops.prior_embed(z.cuda(), *dev).cpu()
    assert torch.equal(bits(got), bits(ref))
    # token 0 of EVERY clip is y_cond (clip 1 must not read the last code of clip 0), and the last code of a clip is never used
    assert torch.equal(got[:, 0], ((y_cond + pos_emb[0]) + x_cond[0]).expand(n, -1))
    z2 = z.clone()
    z2[:, -1] = (z[:, -1] + 3) % bins
    assert not torch.equal(x_emb[z2[0, -1]], x_emb[z[0, -1].clamp(0, bins - 1)])
    assert torch.equal(bits(ops.prior_embed(z2.cuda(), *dev).cpu()), bits(got))
    assert torch.equal(got[0, 2], (x_emb[0] + pos_emb[2]) + x_cond[2])                         # code -3 -> row 0


@pytest.mark.parametrize("with_pred", [True, False], ids=["pred", "nopred"])
@pytest.mark.parametrize("width", [8, 520, 5128, 8192])
def test_prior_head_is_bit_equal_to_the_three_kernels(width, with_pred):
    """NG = 1, 4, 16 and 16 at width 8192: exactly 64 KiB of dynamic LDS"""
    from llark_amd import ops
    n, t, bins = 2, 3, 5
    rows, ldo = n * t, width + 8
    z, x_emb, pos_emb, x_cond, y_cond = (a.cuda() for a in _embed_inputs(n, t, width, bins, 2))
    g = gen(width, 9)
    gamma, beta = (1 + 0.1 * torch.randn(width, generator=g)).cuda(), (0.1 * torch.randn(width, generator=g)).cuda()
    assert ops.prior_head_takes(width, ldo)
    h_ref = ops.prior_embed(z, x_emb, pos_emb, x_cond, y_cond)
    assert torch.equal(bits(h_ref), bits(_embed_torch(*(a.cpu() for a in (z, x_emb, pos_emb, x_cond, y_cond)))))
    s0 = f16_sentinel((rows, ldo))
    hi_ref, lo_ref, hi, lo = s0.cuda(), s0.cuda(), s0.cuda(), s0.cuda()
    ops.layernorm_split(h_ref.view(rows, width), gamma, beta, R.LN_EPS, hi_ref, lo_ref)
    p0 = torch.full((rows, 2), float("nan"))
    pred_ref, pred = p0.cuda(), (p0.cuda() if with_pred else None)
    ops.ln_row_pred(h_ref.view(rows, width), R.LN_EPS, pred_ref)
    h = ops.prior_head(z, x_emb, pos_emb, x_cond, y_cond, gamma, beta, R.LN_EPS, hi, lo, pred)
    _sync()
    assert torch.equal(bits(h), bits(h_ref)), "h differs from prior_embed"
    assert torch.equal(bits(hi), bits(hi_ref)) and torch.equal(bits(lo), bits(lo_ref)), "the planes differ from layernorm_split"
    assert_untouched("hi", hi, s0, mask(s0.shape, rows, 0, width))
    assert_untouched("lo", lo, s0, mask(s0.shape, rows, 0, width))
    assert bool(torch.isfinite(hi[:, :width].float()).all()) and bool((lo[:, :width] != 0).any())
    if with_pred:
        assert bool(torch.isfinite(pred_ref).all()) and torch.equal(bits(pred), bits(pred_ref)), "pred differs from ln_row_pred"


@pytest.mark.parametrize("rows", R.PRED_ROWS)
@pytest.mark.parametrize("width", R.PRED_WIDTHS)
def test_ln_row_pred_mean_and_power_of_two_scale(rows, width):
    from llark_amd import ops
    x = R.pred_inputs(rows, width)
    assert R.pred_margin(x) >= R.PRED_MARGIN, "a row sits on the rounding edge of its scale: the exact comparison below would be a coin toss"
    mean, rstd, l2 = R.pred_reference(x)
    xb = nan_buf(rows, width + 4)
    xb[:, :width] = x
    xg = xb.cuda()
    pred = torch.full((rows + 1, 2), float("nan")).cuda()
    ops.ln_row_pred(xg[:, :width], R.LN_EPS, pred)
    _sync()
    got = pred.cpu()
    assert bool(torch.isnan(got[rows]).all()) and torch.equal(bits(xg), bits(xb))
    atol, r = tol("row mean", x.mean(-1), mean, x.double().abs().mean(-1))
    R.check_frac(f"ln_row_pred mean [{rows}x{width}]", got[:rows, 0], mean, atol, r)
    assert torch.equal(got[:rows, 1].double(), torch.exp2(torch.round(l2))), (got[:rows, 1], rstd)


# =====================================================================================================================
# 4. pooling, zero_pad16
# =====================================================================================================================
@pytest.mark.parametrize("n,t,width,frame_len,frames", R.POOL_WINDOW_SHAPES, ids=lambda v: str(v))
def test_pool_window_matches_float64(n, t, width, frame_len, frames):
    from llark_amd import ops
    h = torch.randn(n, t, width, generator=gen(n, t, width, 3)) * 2.0 + 0.5
    h[:, frames * frame_len:] = float("nan")                       # the dropped tail is never read
    got = ops.pool_window(h.cuda(), frame_len, frames).cpu()
    assert got.shape == (n, frames, width)
    for c in range(n):
        for f in range(frames):
            ref, atol = R.pool_bound(h[c, f * frame_len:(f + 1) * frame_len].double(), frame_len)
            R.report_close(f"pool_window clip {c} frame {f}", got[c, f].double().numpy(), ref.numpy(), atol)


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "nolens"])
@pytest.mark.parametrize("width", R.POOL_MEAN_WIDTHS)
def test_pool_mean_matches_float64(width, with_lens):
    from llark_amd import ops
    n, t = 3, 50
    lens = (t, 1, 37) if with_lens else (t, t, t)
    h = torch.randn(n, t, width, generator=gen(width, 4)) * 2.0 + 0.5
    for c, L in enumerate(lens):
        h[c, L:] = float("nan")
    got = ops.pool_mean(h.cuda(), torch.tensor(lens, dtype=torch.int32).cuda() if with_lens else None).cpu()
    for c, L in enumerate(lens):
        ref, atol = R.pool_bound(h[c, :L].double(), L)
        R.report_close(f"pool_mean clip {c} len {L}", got[c].double().numpy(), ref.numpy(), atol)


@pytest.mark.parametrize("rows,ld,start", [(5, 40, 33), (3, 32, 0), (4, 16, 16), (70000, 24, 8)], ids=lambda v: str(v))
def test_zero_pad16_zeroes_the_pad_and_nothing_else(rows, ld, start):
    """(70000, 24, 8): 1 120 000 pad elements, more than the 4096 x 256 threads of the capped grid; (4, 16, 16): from == ld is a no-op"""
    from llark_amd import ops
    before = torch.randint(1, 2 ** 15 - 1, (rows, ld), generator=gen(rows, ld), dtype=torch.int16)
    plane = before.cuda()
    ops.zero_pad16(plane, start)
    _sync()
    after = plane.cpu()
    assert not bool(after[:, start:].any()) and torch.equal(after[:, :start], before[:, :start])


def test_zero_pad16_refuses_from_past_ld():
    from llark_amd import _lib, ops
    before = torch.full((4, 16), 0x1234, dtype=torch.int16)
    plane = before.cuda()
    with pytest.raises(_lib.LlarkHipError):
        ops.zero_pad16(plane, 17)
    _sync()
    assert torch.equal(plane.cpu(), before)
