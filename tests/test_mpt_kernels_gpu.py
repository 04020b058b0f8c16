"""The MPT / shared training glue kernels, one kernel at a time, against float64 references built on the CPU with plain torch.

Whole-model tests (tests/test_mpt_gpu.py) run these kernels only at d_model 256 and accept 5e-2 over a tensor; here every
kernel is compared element by element at the widths that select each template instantiation, on both sides of every
dispatch edge, with padding / neighbouring memory pre-filled with a sentinel and asserted bit-unchanged afterwards.

Tolerances
----------
* exact kernels (gathers, transposes, clamp, masks, duplicate planes): ``torch.equal``.
* one bf16 plane: ``|got - ref64| <= 2**-8 |ref64| + floor``; hi + lo planes: ``2e-5 max|ref|`` (the figure of
  tests/test_fuzz_gpu.py), and where the values span many magnitudes (GELU / ReLU) additionally never more than
  ``2**-16 |ref64| + floor`` per element (hi carries 8 bits, lo 8 more: the pair is within 2**-17 relative).
  ``floor`` is the fp32 bound below of the value being rounded; under bf16's normal range (2**-126) one ulp is the absolute 2**-133.
* fp32 outputs of reductions: ``c * 2**-24 * B`` with ``B`` the float64 sum of the absolute values of the terms that enter the
  output element and ``c = max(16, 4 * r_torch)``, ``r_torch`` = the worst ``|torch_fp32 - ref64| / (2**-24 B)`` of torch's own
  float32 CPU implementation on the same inputs, measured inside each test (``_tol``) - never taken from the kernel.

``B`` per kernel: layernorm_bwd ``dgamma[c]``: ``sum_r |dy xhat|`` (+ |initial|); ``dbeta[c]``: ``sum_r |dy|`` (+ |initial|);
``dx``: ``rstd (|g| + mean|g| + |xhat| mean|g xhat|)`` (+ |initial| when accumulating), g = dy gamma.  LayerNorm forward:
``rstd |gamma| (|x| + mean|x|) + |beta|``.  GELU: ``|x|``; its derivative: ``|dact| (0.5 (1 + |erf|) + |u| phi(u))`` (>= 0.5 |dact|,
which is the absolute floor the far negative tail needs: there the true value is ~1e-9 |dact| and 1 + erf cancels to one
fp32 ulp of 1).  colsum / scatter-add: ``sum |terms|`` + |initial|.  softmax: ``p (|s| + |bias| + |max| + 2)``.

Measured worst ratios, in units of 2**-24 B, over the cases of this file (torch = its float32 CPU result, kernel = MI355X):

    output                         torch     kernel
    layernorm_bwd dx               8.6       4.6         (c = 34 at [1000x4]; 16 elsewhere)
    layernorm_bwd dgamma           6.0       4.0
    layernorm_bwd dbeta            2.7       2.4
    layernorm_bwd dx, mean 1e3     8.9e2     1.6e2       (the rounding of the mean itself, amplified by rstd, is not in B: torch
    layernorm_bwd dgamma, mean 1e3 4.6e3     2.4e3        pays it too - which is why c is measured and not assumed)
    layernorm_f32_                 3.6       3.7
    gelu (forward, fp32 floor)     6.0       -           (only the bf16 planes exist)
    gelu_bwd fp32                  8.8       3.0
    colsum_add, zero mean          1.3       1.3
    colsum_add, column mean 2      3.8       3.9         (the former one-thread-per-column serial sum: 86.9 at 16384 rows, 42 at
                                                          2968 rows, against c = 16: the reason for the blocked sum in train.hip)
    scatter_add_rows               2.7       1.9
    causal softmax                 < 1       -           (bf16 output: its 2**-8 dominates)

``-s`` prints each test's own figures ("[ratio] ...").
"""
import math

import numpy as np
import pytest
import torch

from kernel_util import assert_untouched as _assert_untouched, bf16_ulp as _bf16_ulp, bf_sentinel as _bf_sentinel, bits as _bits, \
    check as _check, gen as _gen, mask as _mask, nan_buf as _nan_buf, tol as _tol

pytestmark = pytest.mark.gpu

# =====================================================================================================================
# 1. layernorm_bwd
# =====================================================================================================================
LNB_WIDTHS = [4, 60, 256, 260, 1024, 1028, 2048, 2052, 4096]           # NV=1 | 4 | 8 | 16 and both sides of every edge
LNB_ROWS = [1, 3, 4, 5, 37, 1000, 2968]
LNB_SHAPES = sorted({(r, w) for w in LNB_WIDTHS for r in (5, 1000)} | {(r, w) for r in LNB_ROWS for w in (256, 2048)})
LN_EPS = 1e-5


def _lnb_reference(x, gamma, dy, dx0, dg0, db0):
    """float64 autograd of F.layer_norm + the bound B of every output element"""
    x64, g64, dy64 = x.double().requires_grad_(True), gamma.double().requires_grad_(True), dy.double()
    b64 = torch.zeros_like(g64, requires_grad=True)
    y = torch.nn.functional.layer_norm(x64, (x.shape[1],), g64, b64, LN_EPS)
    y.backward(dy64)
    with torch.no_grad():
        mean = x64.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + LN_EPS)
        xh = (x64 - mean) * rstd
        g = dy64 * g64
        b_dx = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)) + dx0.double().abs()
        b_dg = (dy64 * xh).abs().sum(0) + dg0.double().abs()
        b_db = dy64.abs().sum(0) + db0.double().abs()
    return (x64.grad + dx0.double(), g64.grad + dg0.double(), b64.grad + db0.double()), (b_dx, b_dg, b_db)


def _lnb_torch32(x, gamma, dy, dx0, dg0, db0):
    x32, g32 = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    b32 = torch.zeros_like(g32, requires_grad=True)
    torch.nn.functional.layer_norm(x32, (x.shape[1],), g32, b32, LN_EPS).backward(dy)
    return x32.grad + dx0, g32.grad + dg0, b32.grad + db0


def _run_lnb(name, x, gamma, dy, variant):
    from llark_amd import ops
    rows, width = x.shape
    g = _gen(rows, width, 99)
    accumulate = variant in ("acc", "sliced")
    dx0 = torch.randn(rows, width, generator=g) if accumulate else torch.zeros(rows, width)
    dg0, db0 = torch.randn(width, generator=g), torch.randn(width, generator=g)        # the kernel ADDS into dgamma / dbeta
    if variant == "nodbeta":
        db0 = torch.zeros(width)
    (r_dx, r_dg, r_db), (b_dx, b_dg, b_db) = _lnb_reference(x, gamma, dy, dx0, dg0, db0)
    t_dx, t_dg, t_db = _lnb_torch32(x, gamma, dy, dx0, dg0, db0)
    if variant == "sliced":                      # the qk_ln call pattern: three column slices, three leading dimensions
        (ldx, ox), (ldy, oy), (ldd, od) = (3 * width, width), (2 * width + 8, 8), (width + 12, 4)
    else:
        (ldx, ox), (ldy, oy), (ldd, od) = (width, 0), (width, 0), (width, 0)
    pad_rows = rows + 2
    xb, dyb, dxb = _nan_buf(pad_rows, ldx), _nan_buf(pad_rows, ldy), _nan_buf(pad_rows, ldd)
    xb[:rows, ox:ox + width], dyb[:rows, oy:oy + width] = x, dy
    if accumulate:
        dxb[:rows, od:od + width] = dx0
    xg, dyg, dxg = xb.cuda(), dyb.cuda(), dxb.cuda()
    dgg, dbg = dg0.cuda(), (db0.cuda() if variant != "nodbeta" else None)
    ops.layernorm_bwd(xg[:rows, ox:ox + width], gamma.cuda(), dyg[:rows, oy:oy + width], LN_EPS, dxg[:rows, od:od + width], dgg, dbg,
                      accumulate)
    torch.cuda.synchronize()
    _assert_untouched(f"{name} dx buffer", dxg, dxb, _mask(dxb.shape, rows, od, od + width))
    assert torch.equal(_bits(xg), _bits(xb)) and torch.equal(_bits(dyg), _bits(dyb)), f"{name}: an input was modified"
    for nm, got, ref, t32, bnd in (("dx", dxg[:rows, od:od + width], r_dx, t_dx, b_dx), ("dgamma", dgg, r_dg, t_dg, b_dg)) + \
            ((("dbeta", dbg, r_db, t_db, b_db),) if dbg is not None else ()):
        atol, r = _tol(f"layernorm_bwd {nm}", t32.detach(), ref, bnd)
        _check(f"{name} {nm}", got, ref, atol, bound=bnd, r_torch=r)


@pytest.mark.parametrize("variant", ["plain", "acc", "nodbeta", "sliced"])
@pytest.mark.parametrize("rows,width", LNB_SHAPES, ids=lambda v: str(v))
def test_layernorm_bwd_matches_float64_autograd(rows, width, variant):
    """dx / dgamma / dbeta vs float64 autograd of F.layer_norm; NV = 1 (width <= 256), 4 (<= 1024), 8 (<= 2048), 16 (<= 4096)."""
    g = _gen(rows, width, 1)
    x = torch.randn(rows, width, generator=g) * 1.7 + 0.3
    gamma = torch.randn(width, generator=g)
    dy = torch.randn(rows, width, generator=g)
    _run_lnb(f"layernorm_bwd[{rows}x{width} {variant}]", x, gamma, dy, variant)


@pytest.mark.parametrize("rows,width", [(5, 256), (37, 1028), (1000, 2048), (5, 4096)], ids=lambda v: str(v))
@pytest.mark.parametrize("data", ["const_row", "mean1e3"])
def test_layernorm_bwd_degenerate_statistics(rows, width, data):
    """a row of constant x (variance 0: rstd = eps**-0.5) and rows of mean 1e3, spread 1 (cancellation in x - mean)"""
    g = _gen(rows, width, 2)
    x = torch.randn(rows, width, generator=g)
    if data == "const_row":
        x[rows // 2] = 1.5
    else:
        x = x + 1000.0
    gamma = torch.randn(width, generator=g)
    dy = torch.randn(rows, width, generator=g)
    _run_lnb(f"layernorm_bwd[{rows}x{width} {data}]", x, gamma, dy, "plain")


def test_layernorm_bwd_rejects_width_over_4096():
    from llark_amd import _lib, ops
    z = torch.zeros(4, 4100, device="cuda")
    dx = torch.full((4, 4100), float("nan"), device="cuda")
    dg = torch.zeros(4100, device="cuda")
    with pytest.raises(_lib.LlarkHipError, match="too large"):
        ops.layernorm_bwd(z, torch.ones(4100, device="cuda"), z, LN_EPS, dx, dg, None, False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and not bool(dg.any()), "the refused call launched a kernel"


# =====================================================================================================================
# 2. LayerNorm forward: layernorm_bf16, layernorm_bf16_dup, layernorm_f32_
# =====================================================================================================================
LNF_WIDTHS = [4, 252, 256, 260, 1024, 1028, 2048, 2052, 4096, 8192]    # NV = 1 | 4 | 8 | 16 | 32
LNF_SHAPES = sorted({(5, w) for w in LNF_WIDTHS} | {(r, w) for r in (1, 4, 2968) for w in (256, 2048, 8192)})


def _lnf_reference(x, gamma, beta):
    width = x.shape[1]
    x64, g64 = x.double(), gamma.double()
    b64 = beta.double() if beta is not None else None
    ref = torch.nn.functional.layer_norm(x64, (width,), g64, b64, LN_EPS)
    rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + LN_EPS)
    bound = rstd * g64.abs() * (x64.abs() + x64.abs().mean(-1, keepdim=True)) + (b64.abs() if b64 is not None else 0.0)
    t32 = torch.nn.functional.layer_norm(x, (width,), gamma, beta, LN_EPS)
    return ref, bound, t32


def _lnf_inputs(rows, width, with_beta, shift=0.5):
    g = _gen(rows, width, 3)
    x = torch.randn(rows, width, generator=g) * 3 + shift
    return x, torch.randn(width, generator=g), (torch.randn(width, generator=g) if with_beta else None)


@pytest.mark.parametrize("with_beta", [False, True], ids=["nobeta", "beta"])
@pytest.mark.parametrize("entry", ["bf16", "bf16_hi_only", "bf16_dup"])
@pytest.mark.parametrize("rows,width", LNF_SHAPES, ids=lambda v: str(v))
def test_layernorm_forward_bf16_planes(rows, width, entry, with_beta):
    from llark_amd import ops
    x, gamma, beta = _lnf_inputs(rows, width, with_beta)
    ref, bound, t32 = _lnf_reference(x, gamma, beta)
    floor, r = _tol("layernorm fwd", t32, ref, bound)
    name = f"layernorm_{entry}[{rows}x{width} {'beta' if with_beta else 'nobeta'}]"
    bg = beta.cuda() if with_beta else None
    if entry == "bf16_dup":                                   # [hi | lo | hi] column blocks of one K-concatenated operand + pad
        ld = 3 * width + 8
        before = _bf_sentinel((rows + 2, ld))
        buf = before.cuda()
        hi, lo, hi2 = (buf[:rows, k * width:(k + 1) * width] for k in range(3))
        ops.layernorm_bf16_dup(x.cuda(), gamma.cuda(), bg, LN_EPS, hi, lo, hi2)
        torch.cuda.synchronize()
        _assert_untouched(name, buf, before, _mask(before.shape, rows, 0, 3 * width))
        assert torch.equal(_bits(hi), _bits(hi2)), f"{name}: the duplicate plane differs from hi"
    else:
        before = _bf_sentinel((rows + 2, width))
        hb, lb = before.cuda(), before.cuda()
        hi, lo = hb[:rows], (lb[:rows] if entry == "bf16" else None)
        ops.layernorm_bf16(x.cuda(), gamma.cuda(), bg, LN_EPS, hb, lb if entry == "bf16" else None)
        torch.cuda.synchronize()
        for b_ in (hb, lb):
            _assert_untouched(name, b_, before, _mask(before.shape, rows if (b_ is hb or entry == "bf16") else 0, 0, width))
    _check(f"{name} hi", hi.float(), ref, _bf16_ulp(ref) + floor)
    if lo is not None:
        _check(f"{name} hi+lo", hi.float().cpu().double() + lo.float().cpu().double(), ref, 2e-5 * ref.abs().max().item())


@pytest.mark.parametrize("with_beta", [False, True], ids=["nobeta", "beta"])
@pytest.mark.parametrize("rows,width", LNF_SHAPES, ids=lambda v: str(v))
def test_layernorm_f32_in_place_on_qk_column_blocks(rows, width, with_beta):
    """the qk_ln use: in place on the q and the k column block of a [rows][3 D] buffer, the v block bit-unchanged"""
    from llark_amd import ops
    g = _gen(rows, width, 4)
    qkv = torch.randn(rows + 1, 3 * width, generator=g) * 2 + 0.25
    qkv[rows:] = float("nan")
    gq, gk = torch.randn(width, generator=g), torch.randn(width, generator=g)
    bq, bk = (torch.randn(width, generator=g), torch.randn(width, generator=g)) if with_beta else (None, None)
    dev = qkv.cuda()
    ops.layernorm_f32_(dev[:rows, :width], gq.cuda(), bq.cuda() if with_beta else None, LN_EPS)
    ops.layernorm_f32_(dev[:rows, width:2 * width], gk.cuda(), bk.cuda() if with_beta else None, LN_EPS)
    torch.cuda.synchronize()
    _assert_untouched(f"layernorm_f32_[{rows}x{width}]", dev, qkv, _mask(qkv.shape, rows, 0, 2 * width))
    for nm, c0, gam, bet in (("q", 0, gq, bq), ("k", width, gk, bk)):
        ref, bound, t32 = _lnf_reference(qkv[:rows, c0:c0 + width].contiguous(), gam, bet)
        atol, r = _tol("layernorm fwd", t32, ref, bound)
        _check(f"layernorm_f32_[{rows}x{width}] {nm}", dev[:rows, c0:c0 + width], ref, atol, bound=bound, r_torch=r)


def test_layernorm_forward_rejects_width_over_8192():
    from llark_amd import _lib, ops
    x = torch.zeros(4, 8196, device="cuda")
    before = _bf_sentinel((4, 8196))
    hi = before.cuda()
    with pytest.raises(_lib.LlarkHipError, match="too large"):
        ops.layernorm_bf16(x, torch.ones(8196, device="cuda"), None, LN_EPS, hi)
    with pytest.raises(_lib.LlarkHipError, match="too large"):
        ops.layernorm_f32_(x, torch.ones(8196, device="cuda"), None, LN_EPS)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hi), _bits(before)) and not bool(x.any())


# =====================================================================================================================
# 3. exact GELU forward / backward
# =====================================================================================================================
def _gelu_inputs(n, seed):
    """the tails, not only N(0, 1): +-0, +-1e-30, +-40, a grid over [-12, 12] and 3 N(0, 1); a small n takes the specials and an
    evenly spaced subset of the rest (so that 255 values still span the grid), a large n cycles through the set"""
    g = _gen(n, seed)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0])
    rest = torch.cat([torch.linspace(-12, 12, 1537), torch.randn(max(1537, min(n, 1 << 20) - 1543), generator=g) * 3])
    if n <= special.numel():
        return special[:n].contiguous()
    if n < special.numel() + rest.numel():
        pick = torch.linspace(0, rest.numel() - 1, n - special.numel()).round().long()
        return torch.cat([special, rest[pick]]).contiguous()
    base = torch.cat([special, rest])
    return base.repeat(-(-n // base.numel()))[:n].contiguous()


def _gelu64(x64):
    return 0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))


def _gelu_grad64(u64):
    return 0.5 * (1.0 + torch.erf(u64 / math.sqrt(2.0))) + u64 * torch.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("rows,width", [(1, 4), (3, 260), (5, 1024), (37, 8192), (1543, 4), (2968, 8192)], ids=lambda v: str(v))
def test_gelu_split_bf16_matches_float64_erf_gelu(rows, width, with_lo):
    from llark_amd import ops
    x = _gelu_inputs(rows * width, 5).view(rows, width)
    ref = _gelu64(x.double())
    floor, r = _tol("gelu fwd", torch.nn.functional.gelu(x), ref, x.double().abs())
    ld = width + 8                                            # planes = column blocks of a wider buffer, pad columns sentinel
    before = _bf_sentinel((rows + 1, ld))
    hb, lb = before.cuda(), before.cuda()
    ops.gelu_split_bf16(x.cuda(), hb[:rows, :width], lb[:rows, :width] if with_lo else None)
    torch.cuda.synchronize()
    name = f"gelu_split_bf16[{rows}x{width}]"
    _assert_untouched(name, hb, before, _mask(before.shape, rows, 0, width))
    _assert_untouched(name + " lo", lb, before, _mask(before.shape, rows if with_lo else 0, 0, width))
    hi = hb[:rows, :width].float().cpu().double()
    _check(name + " hi", hi, ref, _bf16_ulp(ref) + floor)
    if with_lo:
        both = hi + lb[:rows, :width].float().cpu().double()
        _check(name + " hi+lo", both, ref, np.minimum(2e-5 * ref.abs().max().item(), 2.0 ** -16 * ref.abs().numpy() + floor))


@pytest.mark.parametrize("with_dup32", [False, True], ids=["bf16", "bf16+f32"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2968 * 8192])
def test_gelu_bwd_matches_float64_derivative(n, with_dup32):
    from llark_amd import ops
    u = _gelu_inputs(n, 6)
    g = _gen(n, 7)
    dact = torch.randn(min(n, 1 << 20), generator=g)
    dact = dact.repeat(-(-n // dact.numel()))[:n].roll(7).contiguous()      # not phase-locked with the grid of u
    u64, d64 = u.double(), dact.double()
    ref = d64 * _gelu_grad64(u64)
    bound = d64.abs() * (0.5 * (1.0 + torch.erf(u64 / math.sqrt(2.0)).abs()) + u64.abs() * torch.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi))
    u32 = u.clone().requires_grad_(True)
    torch.nn.functional.gelu(u32).backward(dact)
    atol, r = _tol("gelu bwd", u32.grad, ref, bound)
    del u32
    before16, before32 = _bf_sentinel((n + 5,)), torch.full((n + 5,), float("nan"))
    d16, d32 = before16.cuda(), before32.cuda()
    ops.gelu_bwd(u.cuda(), dact.cuda(), d16[:n], d32[:n] if with_dup32 else None)
    torch.cuda.synchronize()
    written = torch.zeros(n + 5, dtype=torch.bool)
    written[:n] = True
    _assert_untouched("gelu_bwd dup16", d16, before16, written)
    _assert_untouched("gelu_bwd dup32", d32, before32, written if with_dup32 else torch.zeros_like(written))
    if with_dup32:
        _check(f"gelu_bwd[{n}] fp32", d32[:n], ref, atol, bound=bound, r_torch=r)
    _check(f"gelu_bwd[{n}] bf16", d16[:n].float(), ref, _bf16_ulp(ref) + atol)


# =====================================================================================================================
# 4. clamp_f32_, clamp_bwd_bf16_, scale_f32_  (exact)
# =====================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 2968 + 5])
def test_clamp_and_scale_are_bit_exact(n):
    from llark_amd import ops
    g = _gen(n, 8)
    lim = 3.0
    x = torch.randn(n, generator=g) * 2.5
    x[0] = lim
    if n > 4:
        x[1], x[2], x[3], x[4] = -lim, float("nan"), 5.0, -0.0
    before = torch.full((n + 3,), float("nan"))
    buf = before.clone()
    buf[:n] = x
    dev = buf.cuda()
    ops.clamp_f32_(dev[:n], lim)
    written = torch.zeros(n + 3, dtype=torch.bool)
    written[:n] = True
    _assert_untouched("clamp_f32_", dev, before, written)
    want = torch.clamp(x, -lim, lim)                                         # NaN stays NaN, as in the reference's qkv.clamp_
    assert torch.equal(_bits(dev[:n]), _bits(want)), f"clamp_f32_ differs from torch.clamp at {(_bits(dev[:n]) != _bits(want)).nonzero().flatten()[:8].tolist()}"
    # backward: torch's own autograd is the reference (gradient passes at exactly +-limit, 0 at NaN)
    xr = x.clone().requires_grad_(True)
    dy = torch.randn(n, generator=g).bfloat16()
    torch.clamp(xr, -lim, lim).backward(dy.float())
    want_g = xr.grad.bfloat16()
    b16 = _bf_sentinel((n + 3,))
    d16 = b16.clone()
    d16[:n] = dy
    d16g = d16.cuda()
    ops.clamp_bwd_bf16_(x.cuda(), lim, d16g[:n])
    _assert_untouched("clamp_bwd_bf16_", d16g, b16, written)
    assert torch.equal(d16g[:n].cpu().float(), want_g.float()), "clamp_bwd_bf16_ differs from torch.clamp's autograd"
    if n > 4:
        assert d16g[:5].cpu().float().tolist()[:4] == [dy[0].item(), dy[1].item(), 0.0, 0.0]
    # scale
    y = torch.randn(n, generator=g) * 7
    buf = before.clone()
    buf[:n] = y
    dev = buf.cuda()
    ops.scale_f32_(dev[:n], 0.37)
    _assert_untouched("scale_f32_", dev, before, written)
    assert torch.equal(_bits(dev[:n]), _bits(y * 0.37)), "scale_f32_ differs from torch's fp32 product"


# =====================================================================================================================
# 5. causal_softmax_rows_alibi
# =====================================================================================================================
@pytest.mark.parametrize("pad", [False, True], ids=["ldpS", "ldp64"])
@pytest.mark.parametrize("S,nh", [(1, 1), (2, 3), (63, 16), (64, 1), (64, 3), (65, 16), (130, 3), (130, 16), (1000, 3), (1000, 1)], ids=lambda v: str(v))
def test_causal_softmax_rows_alibi_matches_float64(S, nh, pad):
    from llark_amd import ops
    batch = 2 * nh if S < 1000 else nh
    g = _gen(S, nh, 9)
    sc = torch.randn(batch, S, S, generator=g) * 4
    sc[:, S // 4] = sc[:, S // 4] * 0.02 + 800.0           # scale 1/8: a row around +100 (exp overflows fp32 without the max),
    sc[:, S // 2] = sc[:, S // 2] * 0.02 + 640.0           # rows around +80 and -80 (the sum overflows / everything underflows)
    sc[:, S // 3] = sc[:, S // 3] * 0.02 - 640.0
    scale = 0.125
    slopes = 1.0 / torch.pow(2, torch.arange(1, nh + 1, dtype=torch.float32) * (8.0 / nh))
    ldp = -(-S // 64) * 64 if pad else S
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    j = torch.arange(S, dtype=torch.float64)
    bias = slopes.double()[torch.arange(batch) % nh].view(batch, 1, 1) * (j - (S - 1)).view(1, 1, S)
    arg = (sc.double() * scale + bias).masked_fill(~causal, float("-inf"))
    ref = torch.softmax(arg, dim=-1)
    mx = arg.max(-1, keepdim=True).values
    bound = ref * ((sc.double() * scale).abs() + bias.abs() + mx.abs() + 2.0)
    t32 = torch.softmax((sc * scale + bias.float()).masked_fill(~causal, float("-inf")), dim=-1)
    floor, r = _tol("softmax", t32, ref, bound)
    before = _bf_sentinel((batch + 1, S, ldp))
    p = before.cuda()
    ops.causal_softmax_rows_alibi(sc.cuda(), batch, S, scale, slopes.cuda(), nh, p[:batch])
    torch.cuda.synchronize()
    written = torch.zeros(before.shape, dtype=torch.bool)
    written[:batch] = True
    _assert_untouched("causal_softmax_rows_alibi", p, before, written)
    got = p[:batch].cpu()
    dead = torch.ones(S, ldp, dtype=torch.bool)
    dead[:, :S] = ~causal
    assert not bool(_bits(got)[:, dead].any()), "entries above the diagonal / pad columns must be exact zeros"
    _check(f"causal_softmax_rows_alibi[S{S} nh{nh}]", got[:, :, :S].float(), ref, _bf16_ulp(ref) + floor)
    # all slopes 0 == the bias-free kernel, bit for bit
    p0, p1 = torch.zeros((batch, S, ldp), dtype=torch.bfloat16, device="cuda"), torch.ones((batch, S, ldp), dtype=torch.bfloat16, device="cuda")
    ops.causal_softmax_rows_alibi(sc.cuda(), batch, S, scale, torch.zeros(nh, device="cuda"), nh, p0)
    ops.causal_softmax_rows(sc.cuda(), batch, S, scale, p1)
    assert torch.equal(_bits(p0), _bits(p1)), "slopes = 0 must reproduce causal_softmax_rows"


# =====================================================================================================================
# 6. colsum_add, gather_rows, scatter_add_rows, embed_gather, transpose16 / transposed16, split_heads16
# =====================================================================================================================
@pytest.mark.parametrize("data", ["zero_mean", "mean2"])
@pytest.mark.parametrize("rows", [1, 48, 2968, 16384])
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 2048, 8192])
def test_colsum_add_matches_float64_sum(rows, cols, data):
    """out[c] += sum_r x[r][c] on a [rows][ld > cols] buffer; ``mean2``: same-sign terms (a bias gradient need not have zero mean),
    the case where a serial fp32 sum drifts by ~sqrt(rows) ulps"""
    from llark_amd import _lib, ops
    g = _gen(rows, cols, 10)
    ld = cols + 5
    x = torch.randn(rows, cols, generator=g) + (2.0 if data == "mean2" else 0.0)
    out0 = torch.randn(cols, generator=g)
    xb = _nan_buf(rows + 1, ld)
    xb[:rows, :cols] = x
    ob = torch.full((cols + 4,), float("nan"))
    ob[:cols] = out0
    xg, og = xb.cuda(), ob.cuda()
    ops.check(_lib.lib().llark_colsum_f32(xg.data_ptr(), ld, rows, cols, og.data_ptr(), torch.cuda.current_stream().cuda_stream), "colsum")
    torch.cuda.synchronize()
    written = torch.zeros(cols + 4, dtype=torch.bool)
    written[:cols] = True
    _assert_untouched("colsum_add out", og, ob, written)
    assert torch.equal(_bits(xg), _bits(xb))
    ref = x.double().sum(0) + out0.double()
    bound = x.double().abs().sum(0) + out0.double().abs()
    atol, r = _tol("colsum", x.sum(0) + out0, ref, bound)
    _check(f"colsum_add[{rows}x{cols} {data}]", og[:cols], ref, atol, bound=bound, r_torch=r)
    # the wrapper on a contiguous matrix (what the trainers pass) gives the same sum
    og2 = out0.cuda()
    ops.colsum_add(x.cuda(), og2)
    _check(f"colsum_add wrapper[{rows}x{cols} {data}]", og2, ref, atol)


def _index_vectors(n, n_dst, g):
    perm = torch.randperm(n_dst, generator=g)[:n]
    half = perm.clone()
    half[1::2] = half[0::2][: half[1::2].numel()]
    return {"all_equal": torch.full((n,), n_dst // 2, dtype=torch.int64), "permutation": perm, "half_duplicates": half}


@pytest.mark.parametrize("cols", [1, 256, 257, 2048])
@pytest.mark.parametrize("kind", ["all_equal", "permutation", "half_duplicates"])
def test_gather_and_scatter_add_rows(cols, kind):
    from llark_amd import _lib, ops
    n, n_dst = 192, 301
    g = _gen(cols, len(kind), 11)
    idx = _index_vectors(n, n_dst, g)[kind]
    st = torch.cuda.current_stream().cuda_stream
    # ---- gather: dst[i] = src[idx[i]], exact, ld > cols on both sides ----
    lds, ldd = cols + 3, cols + 7
    src = _nan_buf(n_dst, lds)
    src[:, :cols] = torch.randn(n_dst, cols, generator=g)
    dstb = _nan_buf(n + 2, ldd)
    dg, srcg, idxg = dstb.cuda(), src.cuda(), idx.cuda()                       # named: the raw pointers must outlive the launch
    ops.check(_lib.lib().llark_gather_rows_f32(srcg.data_ptr(), lds, idxg.data_ptr(), n, cols, dg.data_ptr(), ldd, st), "gather_rows")
    torch.cuda.synchronize()
    _assert_untouched("gather_rows", dg, dstb, _mask(dstb.shape, n, 0, cols))
    assert torch.equal(_bits(dg[:n, :cols]), _bits(src[idx, :cols])), "gather_rows is not an exact row gather"
    cont = torch.empty((n, cols), device="cuda")
    ops.gather_rows(src[:, :cols].contiguous().cuda(), idx.cuda(), cont)
    assert torch.equal(_bits(cont), _bits(src[idx, :cols]))
    # ---- scatter-add: dst[idx[i]] += src[i] vs float64 index_add_; rows no index names stay bit-unchanged ----
    upd = torch.randn(n, cols, generator=g)
    ub = _nan_buf(n + 1, lds)
    ub[:n, :cols] = upd
    d0 = torch.randn(n_dst, cols, generator=g)
    db = _nan_buf(n_dst + 1, ldd)
    db[:n_dst, :cols] = d0
    dg, ug = db.cuda(), ub.cuda()
    ops.check(_lib.lib().llark_scatter_add_rows_f32(ug.data_ptr(), lds, idxg.data_ptr(), n, cols, dg.data_ptr(), ldd, st), "scatter_add_rows")
    torch.cuda.synchronize()
    hit = torch.zeros(db.shape, dtype=torch.bool)
    hit[idx, :cols] = True
    _assert_untouched("scatter_add_rows", dg, db, hit)
    ref = d0.double().index_add_(0, idx, upd.double())
    bound = d0.double().abs().index_add_(0, idx, upd.double().abs())
    atol, r = _tol("index_add", d0.clone().index_add_(0, idx, upd), ref, bound)
    _check(f"scatter_add_rows[{cols} {kind}]", dg[:n_dst, :cols], ref, atol, bound=bound, r_torch=r)
    cont = d0.cuda()
    ops.scatter_add_rows(upd.cuda(), idx.cuda(), cont)
    _check(f"scatter_add_rows wrapper[{cols} {kind}]", cont, ref, atol)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_embed_gather_is_exact(dtype):
    from llark_amd import ops
    g = _gen(12, dtype.itemsize)
    vocab, width, rows = 131, 260, 77
    table = torch.randn(vocab, width, generator=g).to(dtype)
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[0], ids[1] = 0, vocab - 1
    before = _nan_buf(rows + 1, width + 4)
    out = before.cuda()
    ops.embed_gather(ids.cuda(), table.cuda(), out[:rows])
    torch.cuda.synchronize()
    _assert_untouched("embed_gather", out, before, _mask(before.shape, rows, 0, width))
    assert torch.equal(_bits(out[:rows, :width]), _bits(table[ids].float()))


TR_SIDES = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rows", TR_SIDES)
@pytest.mark.parametrize("cols", TR_SIDES)
def test_transpose16_is_bit_exact_with_zero_padding(rows, cols, dtype):
    from llark_amd import ops
    g = _gen(rows, cols, 13)
    ld_src, ld_dst = cols + 3, -(-rows // 64) * 64
    src = torch.randint(-32768, 32767, (rows, ld_src), generator=g, dtype=torch.int16).view(dtype)      # any bit pattern, NaNs included
    before = torch.full((cols + 1, ld_dst), 0x1234, dtype=torch.int16).view(dtype)
    dst = before.cuda()
    ops.transpose16(src.cuda(), ld_src, rows, cols, dst, ld_dst)
    torch.cuda.synchronize()
    _assert_untouched("transpose16", dst, before, _mask(before.shape, cols, 0, ld_dst))
    want = torch.zeros((cols, ld_dst), dtype=torch.int16)
    want[:, :rows] = _bits(src)[:, :cols].t()
    assert torch.equal(_bits(dst[:cols]), want), "transpose16: wrong element or non-zero padding"
    t = ops.transposed16(src[:, :cols].contiguous().cuda())
    assert t.shape == (cols, ld_dst) and torch.equal(_bits(t), want)


@pytest.mark.parametrize("S,smax", [(24, 64), (93, 96), (96, 96), (130, 192)])
def test_transpose16_batched_vt_cache_strides(S, smax):
    """the MPT trainer's call: vt_cache [BH][128][smax] -> v [BH][S][128], S < smax, batch strides 128 smax / S 128"""
    from llark_amd import ops
    BH = 6
    g = _gen(S, smax, 14)
    vt = torch.randint(-32768, 32767, (BH, 128, smax), generator=g, dtype=torch.int16).view(torch.bfloat16)
    before = _bf_sentinel((BH + 1, S, 128))
    out = before.cuda()
    ops.transpose16(vt.cuda(), smax, 128, S, out, 128, BH, 128 * smax, S * 128)
    torch.cuda.synchronize()
    written = torch.zeros(before.shape, dtype=torch.bool)
    written[:BH] = True
    _assert_untouched("transpose16 batched", out, before, written)
    assert torch.equal(_bits(out[:BH]), _bits(vt)[:, :, :S].transpose(1, 2).contiguous())


@pytest.mark.parametrize("B,S,nh,hd", [(1, 1, 1, 128), (2, 93, 16, 128), (3, 7, 5, 64), (2, 96, 2, 128)], ids=lambda v: str(v))
def test_split_heads16_is_an_exact_permutation(B, S, nh, hd):
    from llark_amd import ops
    g = _gen(B, S, nh, hd, 15)
    x = torch.randint(-32768, 32767, (B * S, nh * hd), generator=g, dtype=torch.int16).view(torch.bfloat16)
    before = _bf_sentinel((B * nh * S * hd + 16,))
    out = before.cuda()
    ops.split_heads16(x.cuda(), B, S, nh, hd, out)
    torch.cuda.synchronize()
    written = torch.zeros(before.shape, dtype=torch.bool)
    written[: B * nh * S * hd] = True
    _assert_untouched("split_heads16", out, before, written)
    want = _bits(x).view(B, S, nh, hd).permute(0, 2, 1, 3).contiguous().view(-1)
    assert torch.equal(_bits(out[: want.numel()]), want)


# =====================================================================================================================
# 7. row counts past 65535 (16 CLAP clips = 65536 first-stage tokens; a 32 x 2048 MPT micro-batch = 65536 rows)
# =====================================================================================================================
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("kernel", ["gelu_split_bf16", "relu_split_bf16"])
def test_row_kernels_take_more_than_65535_rows(kernel, width):
    from llark_amd import ops
    rows = 70000
    x = _gelu_inputs(rows * width, 16).view(rows, width)
    x64 = x.double()
    ref = _gelu64(x64) if kernel == "gelu_split_bf16" else torch.relu(x64)
    t32 = torch.nn.functional.gelu(x) if kernel == "gelu_split_bf16" else torch.relu(x)
    floor, r = _tol("gelu fwd", t32, ref, x64.abs())
    before = _bf_sentinel((rows + 1, width))
    hb, lb = before.cuda(), before.cuda()
    getattr(ops, kernel)(x.cuda(), hb[:rows], lb[:rows])
    torch.cuda.synchronize()
    for b_ in (hb, lb):
        _assert_untouched(kernel, b_, before, _mask(before.shape, rows, 0, width))
    hi = hb[:rows].float().cpu().double()
    _check(f"{kernel}[{rows}x{width}] hi", hi, ref, _bf16_ulp(ref) + floor)
    _check(f"{kernel}[{rows}x{width}] hi+lo", hi + lb[:rows].float().cpu().double(), ref,
           np.minimum(2e-5 * ref.abs().max().item(), 2.0 ** -16 * ref.abs().numpy() + floor))
