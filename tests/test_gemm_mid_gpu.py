"""GPU parity: llark_gemm16_mid (csrc/gemm_mid.hip), the decode-step Linear for 17 .. 64 rows, vs a torch fp64 product of the same bf16
operands -- what nn.Linear computes for one new token of each of 17 .. 64 sequences under LlamaModel.forward.

Operands and bounds are those of tests/test_gemv_dma_gpu.py: a = randn, planes hi = bf16(a), lo = bf16(a - hi), w = 0.05 randn in bf16;
bf16 x bf16 products are exact in fp32 and the kernel adds them in fp32 in its own order: |err| <= 4e-6 * sum_k |a||w| + the bias' /
residual's own rounding.  SwiGLU output is bf16 (one ulp, 2^-8) or hi + lo planes (2^-15), + 1e-5 absolute.

Every output lives inside a NaN / sentinel buffer with a row stride larger than the logical width and rows past m: nothing but the m x n
result may change.  Rows are independent bit for bit: a row's result does not depend on m, on the other rows or on the launch."""
import functools

import pytest
import torch

from kernel_util import assert_untouched, bf_sentinel, bits, mask, nan_buf

pytestmark = pytest.mark.gpu

SHAPES = [(17, 80, 32), (32, 100, 96), (33, 256, 512), (48, 640, 4104 - 8), (63, 16, 11008), (64, 4096, 4096), (64, 32004, 512),
          (20, 12288, 4096)]
SWIGLU_SHAPES = [(17, 96, 512), (40, 1024, 4096), (64, 11008, 4096)]
PAD_ROWS, PAD_COLS = 3, 5


def _planes(a):
    hi = a.bfloat16()
    lo = (a - hi.float()).bfloat16()
    return hi, lo


def _padded_a(x):
    """x bf16 [m][k] as a view of a [m + 2][k + 8] buffer whose other elements are NaN: lda > k, rows >= m exist and are poison"""
    m, k = x.shape
    buf = torch.full((m + 2, k + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[:m, :k] = x
    return buf[:m, :k]


def _scratch(m, n, k, split, epi):
    from llark_amd import ops
    need = ops.gemm16_mid_scratch_bytes(m, n, k, split, epi)
    assert need > 0
    return torch.full((need // 4,), float("nan"), device="cuda")          # the kernel may not rely on what the scratch holds


@functools.lru_cache(maxsize=2)
def _operands(m, n, k):
    g = torch.Generator(device="cuda").manual_seed(m * 100 + n)
    a = torch.randn(m, k, generator=g, device="cuda")
    w = (torch.randn(n, k, generator=g, device="cuda") * 0.05).bfloat16()
    bias = torch.randn(n, generator=g, device="cuda")
    r0 = torch.randn(m, n, generator=g, device="cuda")
    hi, lo = _planes(a)
    out = {"w": w, "bias": bias, "r0": r0, "hi": _padded_a(hi), "lo": _padded_a(lo)}
    for split in (True, False):
        aeff = (hi.float() + lo.float()) if split else hi.float()
        out[split] = (aeff.double() @ w.double().t(), aeff.double().abs() @ w.double().abs().t())      # reference, sum_k |a||w|
    return out


def _worst(name, err, tol):
    r = float((err / tol.clamp_min(1e-300)).max())
    print(f"[ratio] {name}: worst |err| / tolerance = {r:.3g}")
    return r


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_f32_and_residual(split, m, n, k):
    from llark_amd import ops
    o = _operands(m, n, k)
    ref, bound = o[split]
    hi, lo, w, bias, r0 = o["hi"], o["lo"] if split else None, o["w"], o["bias"], o["r0"]
    assert hi.stride(0) > k
    written = mask((m + PAD_ROWS, n + PAD_COLS), m, 1, 1 + n)
    buf = nan_buf(m + PAD_ROWS, n + PAD_COLS).cuda()
    before = buf.clone()
    ops.gemm16_mid(hi, lo, w, bias, n, ops.EPI_F32, _scratch(m, n, k, split, ops.EPI_F32), c=buf[:, 1:1 + n], m=m)
    assert_untouched("F32", buf, before, written)
    c = buf[:m, 1:1 + n].double()
    tol = 4e-6 * bound + 1e-6 * bias.abs().double()
    assert _worst(f"F32 {m}x{n}x{k} split={split}", (c - (ref + bias.double())).abs(), tol) <= 1.0
    buf2 = nan_buf(m + PAD_ROWS, n + PAD_COLS).cuda()
    buf2[:m, 1:1 + n] = r0
    before2 = buf2.clone()
    c2 = buf2[:, 1:1 + n]
    ops.gemm16_mid(hi, lo, w, None, n, ops.EPI_RESID, _scratch(m, n, k, split, ops.EPI_RESID), c=c2, resid=c2, m=m)     # in place
    assert_untouched("RESID", buf2, before2, written)
    tol2 = 4e-6 * bound + 2e-7 * (ref.abs() + r0.abs().double())
    assert _worst(f"RESID {m}x{n}x{k} split={split}", (c2[:m].double() - (ref + r0.double())).abs(), tol2) <= 1.0


def _swiglu_operands(m, inter, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(m, k, generator=g, device="cuda")
    gate = (torch.randn(inter, k, generator=g, device="cuda") * 0.05).bfloat16()
    up = (torch.randn(inter, k, generator=g, device="cuda") * 0.05).bfloat16()
    packed = torch.stack([gate.view(-1, 32, k), up.view(-1, 32, k)], dim=1).reshape(2 * inter, k).contiguous()
    return a, gate, up, packed


def _sentinel_out(m, inter):
    return bf_sentinel((m + PAD_ROWS, inter + PAD_COLS)).cuda()


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("m,inter,k", SWIGLU_SHAPES)
def test_swiglu(split, m, inter, k):
    """gate / up rows interleaved [gate 32 | up 32] per 64 weight rows (the packed layout of the engine)."""
    from llark_amd import ops
    a, gate, up, packed = _swiglu_operands(m, inter, k, inter + m)
    hi, lo = _planes(a)
    aeff = (hi.float() + lo.float()) if split else hi.float()
    ref = torch.nn.functional.silu(aeff.double() @ gate.double().t()) * (aeff.double() @ up.double().t())
    epi = ops.EPI_SWIGLU_SPLIT if split else ops.EPI_SWIGLU16
    oh, ol = _sentinel_out(m, inter), _sentinel_out(m, inter)
    bh, bl = oh.clone(), ol.clone()
    ops.gemm16_mid(_padded_a(hi), _padded_a(lo) if split else None, packed, None, 2 * inter, epi, _scratch(m, 2 * inter, k, split, epi),
                   out_hi=oh[:, 1:1 + inter], out_lo=ol[:, 1:1 + inter] if split else None, m=m)
    written = mask(tuple(oh.shape), m, 1, 1 + inter)
    assert_untouched("SwiGLU hi", oh, bh, written)
    assert_untouched("SwiGLU lo", ol, bl, written if split else torch.zeros_like(written))
    got = oh[:m, 1:1 + inter].double() + (ol[:m, 1:1 + inter].double() if split else 0.0)
    tol = (2 ** -15 if split else 2 ** -8) * ref.abs() + 1e-5
    assert _worst(f"SwiGLU {m}x{inter}x{k} split={split}", (got - ref).abs(), tol) <= 1.0


def _run_resid(hi, lo, w, r0, m):
    from llark_amd import ops
    n, k = w.shape
    c = r0[:m].clone()
    ops.gemm16_mid(hi[:m], None if lo is None else lo[:m], w, None, n, ops.EPI_RESID,
                   _scratch(m, n, k, lo is not None, ops.EPI_RESID), c=c, resid=c, m=m)
    return (bits(c),)


def _run_swiglu(hi, lo, w, r0, m):
    from llark_amd import ops
    n, k = w.shape
    epi = ops.EPI_SWIGLU_SPLIT if lo is not None else ops.EPI_SWIGLU16
    oh = torch.empty((m, n // 2), dtype=torch.bfloat16, device="cuda")
    ol = torch.empty_like(oh) if lo is not None else None
    ops.gemm16_mid(hi[:m], None if lo is None else lo[:m], w, None, n, epi, _scratch(m, n, k, lo is not None, epi), out_hi=oh, out_lo=ol, m=m)
    return (bits(oh),) + ((bits(ol),) if ol is not None else ())


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("kind,n,k", [("resid", 640, 4096), ("resid", 100, 96), ("swiglu", 2048, 4096), ("swiglu", 192, 512)])
def test_rows_are_independent_bit_for_bit(split, kind, n, k):
    """Rows 0 .. 16 of an m = 64 launch == the m = 17 launch on those rows alone == the m = 64 launch with rows 17 .. 63 replaced
    (1e30 values among them) == the same launch again.  Shapes: with and without a K split across workgroups."""
    g = torch.Generator(device="cuda").manual_seed(n + k)
    a = torch.randn(64, k, generator=g, device="cuda")
    w = (torch.randn(n, k, generator=g, device="cuda") * 0.05).bfloat16()
    r0 = torch.randn(64, n, generator=g, device="cuda")
    hi, lo = _planes(a)
    run = _run_resid if kind == "resid" else _run_swiglu
    full = run(hi, lo if split else None, w, r0, 64)
    again = run(hi, lo if split else None, w, r0, 64)
    alone = run(hi, lo if split else None, w, r0, 17)
    a2 = a.clone()
    a2[17:] = torch.randn(47, k, generator=g, device="cuda") * 3.0
    a2[20:24] = 1e30
    a2[40, ::7] = -1e30
    hi2, lo2 = _planes(a2)
    r2 = r0.clone()
    r2[17:] = 1e30
    other = run(hi2, lo2 if split else None, w, r2, 64)
    for x, y in zip(full, again):
        assert torch.equal(x, y), "two identical launches differ"
    for x, y, z in zip(full, alone, other):
        assert torch.equal(x[:17], y), "rows 0..16 depend on m"
        assert torch.equal(x[:17], z[:17]), "rows 0..16 depend on what rows 17..63 hold"
    for mm in (33, 48):                                                  # every row-tile count
        for x, y in zip(full, run(hi, lo if split else None, w, r0, mm)):
            assert torch.equal(x[:mm], y), f"rows depend on m (m = {mm})"


def test_same_result_as_the_tiled_kernel_within_rounding():
    """The path ops.gemm16 takes for 16 < m <= 128 today (128x128x32 tiles, variant 0) and this kernel agree to fp32 rounding."""
    from llark_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    m, n, k = 32, 4096, 4096
    a = torch.randn(m, k, generator=g, device="cuda")
    w = (torch.randn(n, k, generator=g, device="cuda") * 0.05).bfloat16()
    hi, lo = _planes(a)
    c1 = torch.empty(m, n, device="cuda")
    c2 = torch.empty(m, n, device="cuda")
    ops.gemm16_mid(hi, lo, w, None, n, ops.EPI_F32, _scratch(m, n, k, True, ops.EPI_F32), c=c1)
    ops.gemm16(hi, lo, w, None, n, ops.EPI_F32, c=c2)
    d = (c1 - c2).abs().max().item()
    print(f"[ratio] mid vs tiled: max diff {d:.3g} = {d / c2.abs().max().item():.3g} x max|c|")
    assert d <= 2e-5 * c2.abs().max().item()
