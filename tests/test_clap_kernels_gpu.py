"""The CLAP gathers and row kernels (csrc/clap.hip and the shared split / row kernels it uses), one kernel at a time, against
index-exact or float64 references written out in plain torch here.  The whole-model tests (tests/test_clap_gpu.py) see these
kernels only through a 512-vector at 1e-4: an index error that touches one token in a thousand does not move that.

Tolerances as in tests/test_mpt_kernels_gpu.py: gathers and plane splits ``torch.equal``; fp32 reductions ``c 2**-24 B`` with
``c = max(16, 4 r_torch)`` measured on torch's own fp32 CPU result inside the test; bf16 hi + lo planes ``2e-5 max|ref|``, one
plane ``2**-8 |ref| + floor``.  Measured worst ratios in units of 2**-24 B (torch fp32 CPU / kernel): mean_rows_f32 2.3 / 6.7 (a
serial sum of 256 rows), l2_normalize_rows_ 2.1 / 3.0, patchify (fp32 restatement) 3.1; clap_window_attn hi + lo: 4.1e-6
(head_dim 16) and 5.4e-6 (head_dim 32) of max|ref| against the 2e-5 allowed.
"""
import math

import pytest
import torch

from conftest import report_close
from kernel_util import assert_untouched as _assert_untouched, bf16_ulp as _bf16_ulp, bf_sentinel as _bf_sentinel, bits as _bits, check as _check, gen as _gen, \
    mask as _mask, nan_buf as _nan_buf, tol as _tol

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- patch merging ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,H,W,C", [(1, 2, 2, 4), (3, 8, 8, 96), (2, 64, 64, 96), (2, 16, 16, 384), (2, 8, 16, 8)], ids=lambda v: str(v))
def test_clap_patch_merge_is_the_swin_gather(batch, H, W, C):
    """bit-exact against cat([x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2]], -1); the input is arange, so an index
    error shows as a wrong integer; ldx > C, ldo > 4 C with NaN padding that must stay untouched"""
    from llark_amd import _lib, ops
    n = batch * H * W
    ldx, ldo = C + 4, 4 * C + 8
    xb = _nan_buf(n + 1, ldx)
    xb[:n, :C] = torch.arange(n * C, dtype=torch.float32).view(n, C)           # < 2**24: exact integers
    x = xb[:n, :C].view(batch, H, W, C)
    want = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(n // 4, 4 * C)
    ob = _nan_buf(n // 4 + 1, ldo)
    xg, og = xb.cuda(), ob.cuda()
    ops.check(_lib.lib().llark_clap_patch_merge(xg.data_ptr(), ldx, batch, H, W, C, og.data_ptr(), ldo, _stream()), "clap_patch_merge")
    torch.cuda.synchronize()
    _assert_untouched("clap_patch_merge", og, ob, _mask(ob.shape, n // 4, 0, 4 * C))
    got = og[: n // 4, : 4 * C].cpu()
    bad = (got != want).nonzero()
    assert torch.equal(_bits(got), _bits(want)), f"clap_patch_merge: {bad.shape[0]} wrong elements, first at {bad[:1].tolist()}: got {got[tuple(bad[0])].item() if bad.numel() else None}"
    out = torch.empty((n // 4, 4 * C), device="cuda")
    ops.clap_patch_merge(xb[:n, :C].contiguous().cuda(), batch, H, W, out)
    assert torch.equal(_bits(out), _bits(want))


# ---- patchify ----------------------------------------------------------------------------------------------------------
def _patchify_reference(x, mu, sc, bi, idx, w, spec, patch, dtype):
    """BatchNorm over the mel bins -> 4-tap time stretch -> fold the time chunks under each other along frequency -> patch rows"""
    B, T, mel = x.shape
    ratio, G = spec // mel, spec // patch
    xn = (x.to(dtype) - mu.to(dtype)) * sc.to(dtype) + bi.to(dtype)                      # (B, T, mel)
    taps = xn[:, idx.long()]                                                              # (B, spec * ratio, 4, mel)
    st = (w.to(dtype)[None, :, 0, None] * taps[:, :, 0] + w.to(dtype)[None, :, 1, None] * taps[:, :, 1]
          + w.to(dtype)[None, :, 2, None] * taps[:, :, 2] + w.to(dtype)[None, :, 3, None] * taps[:, :, 3])
    img = st.view(B, ratio, spec, mel).permute(0, 1, 3, 2).reshape(B, spec, spec)           # rows: folded frequency, columns: time
    rows = img.view(B, G, patch, G, patch).permute(0, 1, 3, 2, 4).reshape(B * G * G, patch * patch)
    bound = None
    if dtype == torch.float64:
        an = (x.double().abs() + mu.double().abs()) * sc.double().abs() + bi.double().abs()
        ab = (w.double().abs()[None, :, :, None] * an[:, idx.long()]).sum(2)
        ab = ab.view(B, ratio, spec, mel).permute(0, 1, 3, 2).reshape(B, spec, spec)
        bound = ab.view(B, G, patch, G, patch).permute(0, 1, 3, 2, 4).reshape(B * G * G, patch * patch)
    return rows, bound


@pytest.mark.parametrize("taps", ["engine", "one_hot"])
@pytest.mark.parametrize("B,frames,mel,spec", [(2, 100, 8, 32), (1, 128, 8, 32), (2, 1001, 64, 256), (3, 37, 16, 64)], ids=lambda v: str(v))
def test_clap_patchify_matches_restatement(B, frames, mel, spec, taps):
    from llark_amd import ops
    from llark_amd.clap.htsat import bicubic_time_taps
    patch = 4
    g = _gen(B, frames, mel, spec, 21)
    x = torch.randn(B, frames, mel, generator=g) * 20 - 30                               # log-mel dB-like values
    mu, sc, bi = torch.randn(mel, generator=g) * 5 - 30, torch.rand(mel, generator=g) * 0.1 + 0.02, torch.randn(mel, generator=g) * 0.3
    out_frames = spec * (spec // mel)
    if taps == "engine":
        idx, w = (torch.from_numpy(a) for a in bicubic_time_taps(frames, out_frames))
    else:                                                    # one tap of weight 1 at a random position: the kernel is a pure gather
        idx = torch.randint(0, frames, (out_frames, 4), generator=g, dtype=torch.int32)
        w = torch.nn.functional.one_hot(torch.randint(0, 4, (out_frames,), generator=g), 4).float()
    rows = B * (spec // patch) ** 2
    before = _bf_sentinel((rows, 32))
    hi, lo = before.cuda(), before.cuda()
    ops.clap_patchify(x.cuda(), mu.cuda(), sc.cuda(), bi.cuda(), idx.cuda(), w.cuda(), spec, patch, hi, lo)
    torch.cuda.synchronize()
    for p in (hi, lo):
        _assert_untouched("clap_patchify pad columns", p, before, _mask(before.shape, rows, 0, 16))
    name = f"clap_patchify[{B}x{frames}x{mel} {taps}]"
    ref, bound = _patchify_reference(x, mu, sc, bi, idx, w, spec, patch, torch.float64)
    t32, _ = _patchify_reference(x, mu, sc, bi, idx, w, spec, patch, torch.float32)
    floor, r = _tol("patchify", t32, ref, bound)
    h64 = hi[:, :16].float().cpu().double()
    _check(name + " hi", h64, ref, _bf16_ulp(ref) + floor)
    _check(name + " hi+lo", h64 + lo[:, :16].float().cpu().double(), ref, 2e-5 * ref.abs().max().item())
    if taps == "one_hot":                                    # 1 * v + 0 * others is v exactly: both planes bit-exact
        want_hi = t32.bfloat16()
        want_lo = (t32 - want_hi.float()).bfloat16()
        assert torch.equal(hi[:, :16].cpu().float(), want_hi.float()) and torch.equal(lo[:, :16].cpu().float(), want_lo.float()), \
            f"{name}: a one-hot tap table must make the kernel an exact gather"


# ---- token mean, L2 normalisation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,L,C", [(1, 1, 4), (3, 64, 768), (16, 64, 1), (2, 256, 257), (5, 7, 255)], ids=lambda v: str(v))
def test_mean_rows_f32_matches_float64(batch, L, C):
    from llark_amd import _lib, ops
    g = _gen(batch, L, C, 22)
    x = torch.randn(batch * L, C, generator=g) + 0.5
    ldx, ldo = C + 3, C + 5
    xb, ob = _nan_buf(batch * L + 1, ldx), _nan_buf(batch + 1, ldo)
    xb[: batch * L, :C] = x
    xg, og = xb.cuda(), ob.cuda()
    ops.check(_lib.lib().llark_mean_rows_f32(xg.data_ptr(), ldx, batch, L, C, og.data_ptr(), ldo, _stream()), "mean_rows_f32")
    torch.cuda.synchronize()
    _assert_untouched("mean_rows_f32", og, ob, _mask(ob.shape, batch, 0, C))
    ref = x.double().view(batch, L, C).mean(1)
    bound = x.double().abs().view(batch, L, C).mean(1)
    atol, r = _tol("mean_rows", x.view(batch, L, C).mean(1), ref, bound)
    _check(f"mean_rows_f32[{batch}x{L}x{C}]", og[:batch, :C], ref, atol, bound=bound, r_torch=r)
    out = torch.empty((batch, C), device="cuda")
    ops.mean_rows_f32(x.cuda(), batch, out)
    _check(f"mean_rows_f32 wrapper[{batch}x{L}x{C}]", out, ref, atol)


@pytest.mark.parametrize("rows,width", [(1, 1), (3, 63), (4, 64), (5, 65), (9, 512), (2, 8192)], ids=lambda v: str(v))
def test_l2_normalize_rows_matches_f_normalize(rows, width):
    from llark_amd import _lib, ops
    g = _gen(rows, width, 23)
    x = torch.randn(rows, width, generator=g) * 3
    x[rows // 2] = 0.0                                          # an all-zero row stays 0 (no NaN), as F.normalize
    if rows > 2:
        x[0] *= 1e-15                                           # norm^2 far below fp32's normal range is still the row's own scale
    ld = width + 6
    xb = _nan_buf(rows + 1, ld)
    xb[:rows, :width] = x
    xg = xb.cuda()
    ops.check(_lib.lib().llark_l2_normalize_rows(xg.data_ptr(), ld, rows, width, 1e-12, _stream()), "l2_normalize_rows")
    torch.cuda.synchronize()
    _assert_untouched("l2_normalize_rows_", xg, xb, _mask(xb.shape, rows, 0, width))
    ref = torch.nn.functional.normalize(x.double(), dim=-1, eps=1e-12)
    atol, r = _tol("l2_normalize", torch.nn.functional.normalize(x, dim=-1, eps=1e-12), ref, ref.abs())
    _check(f"l2_normalize_rows_[{rows}x{width}]", xg[:rows, :width], ref, atol, bound=ref.abs(), r_torch=r)
    assert not bool(xg[rows // 2, :width].any()), "an all-zero row must stay exactly 0"
    xc = x.cuda()
    ops.l2_normalize_rows_(xc)
    _check(f"l2_normalize_rows_ wrapper[{rows}x{width}]", xc, ref, atol)


# ---- ReLU -> planes, fp32 -> planes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("rows,width", [(1, 1), (3, 255), (5, 257), (2, 1024)], ids=lambda v: str(v))
def test_relu_split_bf16_is_exact(rows, width, with_lo):
    from llark_amd import ops
    g = _gen(rows, width, 24)
    x = torch.randn(rows, width, generator=g) * 5
    x.view(-1)[0] = -0.0
    if width > 4:
        x[:, 1], x[:, 2], x[:, 3] = -1e-30, 1e-30, -7.25
    before = _bf_sentinel((rows + 1, width))
    hb, lb = before.cuda(), before.cuda()
    ops.relu_split_bf16(x.cuda(), hb[:rows], lb[:rows] if with_lo else None)
    torch.cuda.synchronize()
    _assert_untouched("relu_split_bf16 hi", hb, before, _mask(before.shape, rows, 0, width))
    _assert_untouched("relu_split_bf16 lo", lb, before, _mask(before.shape, rows if with_lo else 0, 0, width))
    y = torch.relu(x)
    want_hi = y.bfloat16()
    assert torch.equal(hb[:rows].cpu().float(), want_hi.float()), "relu_split_bf16: hi != bf16(relu(x))"
    assert not bool((hb[:rows].cpu().float() < 0).any())
    if with_lo:
        assert torch.equal(lb[:rows].cpu().float(), (y - want_hi.float()).bfloat16().float()), "relu_split_bf16: lo != bf16(relu(x) - hi)"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("rows,width,ld", [(1, 1, 32), (5, 255, 256), (3, 257, 288), (4, 260, 288), (37, 1024, 1024)], ids=lambda v: str(v))
def test_split16_into_is_exact_and_zero_fills_the_pad_columns(rows, width, ld, with_lo, dtype):
    from llark_amd import ops
    g = _gen(rows, width, ld, 25)
    x = torch.randn(rows, width, generator=g) * 3
    before = torch.full((rows + 1, ld), 0x1234, dtype=torch.int16).view(dtype)
    hb, lb = before.cuda(), before.cuda()
    ops.split16_into(x.cuda(), hb[:rows], lb[:rows] if with_lo else None)
    torch.cuda.synchronize()
    _assert_untouched("split16_into hi", hb, before, _mask(before.shape, rows, 0, ld))
    _assert_untouched("split16_into lo", lb, before, _mask(before.shape, rows if with_lo else 0, 0, ld))
    assert not bool(_bits(hb[:rows, width:]).any()) and not (with_lo and bool(_bits(lb[:rows, width:]).any())), "pad columns [width, ld) must be zero"
    want_hi = x.to(dtype)
    assert torch.equal(_bits(hb[:rows, :width]), _bits(want_hi)), "split16_into: hi != round(x)"
    if with_lo:
        assert torch.equal(lb[:rows, :width].cpu().float(), (x - want_hi.float()).to(dtype).float()), "split16_into: lo != round(x - hi)"


# ---- Swin window attention: both head dims, shifted, H != W -------------------------------------------------------------
def _windows(x, ws):
    """(B, H, W, C) -> (B * H/ws * W/ws, ws * ws, C), windows in row-major order"""
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _window_attention_reference(qkv, B, H, W, C, heads, shift, table):
    """float64 shifted-window attention with the relative-position bias (Swin): roll, partition, softmax(q k^T / sqrt(hd) + bias
    + mask) v, reverse, roll back"""
    ws, hd = 8, C // heads
    x = qkv.double().view(B, H, W, 3 * C)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    win = _windows(x, ws)                                                                  # (nWB, 64, 3C)
    q, k, v = (win[..., i * C:(i + 1) * C].reshape(-1, 64, heads, hd).transpose(1, 2) for i in range(3))
    yy, xx = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    dy = yy.reshape(-1)[:, None] - yy.reshape(-1)[None, :] + ws - 1
    dx = xx.reshape(-1)[:, None] - xx.reshape(-1)[None, :] + ws - 1
    bias = table.double()[(dy * (2 * ws - 1) + dx).view(-1)].view(64, 64, heads).permute(2, 0, 1)
    att = q @ k.transpose(-1, -2) / math.sqrt(hd) + bias
    if shift:
        region = torch.zeros(1, H, W, 1)
        n = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                region[:, hs, wsl] = n
                n += 1
        mw = _windows(region, ws).view(-1, 64)
        mask = (mw[:, None, :] != mw[:, :, None]).double() * -100.0                       # (nW, 64, 64)
        nW = mask.shape[0]
        att = (att.view(B, nW, heads, 64, 64) + mask.view(1, nW, 1, 64, 64)).view(-1, heads, 64, 64)
    ctx = (torch.softmax(att, -1) @ v).transpose(1, 2).reshape(B, H // ws, W // ws, ws, ws, C)
    out = ctx.permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        out = torch.roll(out, (shift, shift), (1, 2))
    return out.reshape(B * H * W, C)


@pytest.mark.parametrize("B,H,W,C,heads,shift", [(2, 16, 32, 32, 2, 4), (1, 32, 16, 64, 4, 4), (2, 24, 16, 16, 1, 4), (1, 16, 16, 32, 2, 0),
                                                 (2, 16, 32, 64, 2, 4), (1, 24, 40, 128, 4, 4), (1, 32, 16, 32, 1, 3), (3, 8, 8, 64, 2, 0)],
                         ids=lambda v: str(v))
def test_clap_window_attn_both_head_dims_shifted_rectangular(B, H, W, C, heads, shift):
    """head_dim 16 (the scalar kernel) and 32 (the MFMA kernel) share no code: each at H != W with shifted windows, against
    float64; planes as column blocks [hi | lo | hi] of one buffer with a sentinel pad"""
    from llark_amd import ops
    assert C // heads in (16, 32)
    g = _gen(B, H, W, C, heads, shift, 26)
    n = B * H * W
    qkv = torch.randn(n, 3 * C, generator=g)
    table = torch.randn(225, heads, generator=g)
    ref = _window_attention_reference(qkv, B, H, W, C, heads, shift, table)
    before = _bf_sentinel((n + 1, 3 * C + 8))
    buf = before.cuda()
    hi, lo, hi2 = (buf[:n, k * C:(k + 1) * C] for k in range(3))
    ops.clap_window_attn(qkv.cuda(), B, H, W, C, heads, 8, shift, table.cuda(), hi, lo, hi2)
    torch.cuda.synchronize()
    _assert_untouched("clap_window_attn", buf, before, _mask(before.shape, n, 0, 3 * C))
    assert torch.equal(_bits(hi), _bits(hi2)), "the duplicate plane differs from hi"
    got = hi.float().cpu().double() + lo.float().cpu().double()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"[ratio] clap_window_attn hd{C // heads} {B}x{H}x{W} shift {shift}: max err / max|ref| = {err:.3g}")
    report_close(f"clap_window_attn hd{C // heads}", got.numpy(), ref.numpy(), 2e-5 * ref.abs().max().item())
