"""References, inputs and bounds for the kernel-level tests of the Llama inference kernels of csrc/llama.hip (attn_prefill_kernel,
attn_decode_kernel, rope_split_kernel, rmsnorm_kernel, embed_gather_kernel).  A plain module: tests/test_llama_kernels_gpu.py runs the
kernels against it, tests/test_llama_kernel_ref_cpu.py proves on the CPU that its bounds reject wrong kernels and accept the
correct arithmetic.

Layout used throughout: N = batch * nh "heads" in launch order (head h of sequence b is n = b * nh + h); q [N][S][128], k / v
[N][T][128] hold the operand VALUES the kernel reads -- the bf16 plane, or float(hi) + float(lo) of the two planes -- nothing is
rounded again on the way into a reference.

Bounds (per output element; ``B = sum_j p_j |v_jd|``, ``A = max_j (scale sum_d |q_d| |k_jd| + |alibi_j|)`` over the visible keys):

    decode                                u + c 2^-24 (1 + 2A) B                    fp32 fma chains, expf
    prefill, bf16 operands, P2            u + (2^-16 + c 2^-24 (1 + 2A)) B          p enters the second product as bf16 hi + lo
    prefill, hi + lo operands (SPLIT)     u + (2^-16 (2 + 2A) + c 2^-24 (1 + 2A)) B  + the two dropped lo.lo products
    prefill _lse (one bf16 p plane)       u + (2^-8 + c 2^-24 (1 + 2A)) B           p rounded to bf16 once
    lse                                   c 2^-24 (1 + |lse| + A)

``u`` = the rounding of the output planes: one bf16 ulp (``kernel_util.bf16_ulp``) for one plane, 2^-16 |ref| for hi + lo.  ``c`` =
``max(16, 4 r)``, ``r`` the worst ratio of torch's own float32 CPU attention on the same operands (``kernel_util.tol``).  A score
error ds changes p_j by p_j ds_j and the normaliser by at most max ds: hence the factor 2A on a relative score error.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from kernel_util import bf16_ulp, check_frac, gen, tol

HD = 128
SCALE = 1.0 / math.sqrt(HD)
GARBAGE = 0x7F7F                      # the largest finite bf16: what cache positions >= total hold in these tests
MODES = ("bf16", "split", "lse")      # prefill: attn_prefill_kernel<SPLIT, NQ, P2, ALIBI> = <0, *, 1, *>, <1, 1, 1, *>, <0, *, 0, *>


def round_up(x, m):
    return (x + m - 1) // m * m


def planes(x):
    """fp32 -> the bf16 hi plane and the bf16 plane of the rounding residual, as store_split writes them"""
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def value(hi, lo=None, dtype=torch.float64):
    """the operand value the kernel reads from one plane or two"""
    return hi.to(dtype) if lo is None else hi.to(dtype) + lo.to(dtype)


def garbage(shape):
    return torch.full(shape, GARBAGE, dtype=torch.int16).view(torch.bfloat16)


def alibi_slopes(nh):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / nh) for h in range(nh)], dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# launcher rules (csrc/llama.hip: launch_attn_prefill, attn_decode)
# ---------------------------------------------------------------------------------------------------------------------
def prefill_rule(batch, nh, s, split):
    """the instantiation and grid llark_attn_prefill_* picks: NQ query sets per wave, query blocks nt, paired workgroups, XCD numbering"""
    nbh = batch * nh
    nq = 2 if (not split and -(-s // 128) * nbh >= 1024) else 1
    nt = -(-s // (64 * nq))
    w = -(-nt // 2) * nbh
    paired = nt >= 2 and (w in (512, 1024) or w >= 2048)
    return SimpleNamespace(nq=nq, nt=nt, paired=paired, xcd=nbh % 8 == 0, workgroups=w if paired else nt * nbh)


def decode_waves(batch, nh):
    return 16 if nh * batch < 256 else 4


# (batch, nh, s, past) -> (NQ, paired, XCD numbering, query blocks nt) with bf16 operands: the smallest shapes that reach every
# branch of the rule.  Paired grids with batch * nh % 8 != 0 need sequences of several thousand positions and are left out.
PREFILL_SHAPES = {
    (1, 3, 130, 0): (1, False, False, 3), (2, 3, 70, 37): (1, False, False, 2), (1, 2, 5, 200): (1, False, False, 1),
    (1, 1, 64, 0): (1, False, False, 1), (1, 2, 65, 63): (1, False, False, 2), (1, 2, 61, 0): (1, False, False, 1),
    (1, 1, 1, 0): (1, False, False, 1),
    (1, 8, 200, 0): (1, False, True, 4), (1, 8, 100, 92): (1, False, True, 2),
    (16, 32, 100, 0): (1, True, True, 2),             # W = 512
    (8, 32, 150, 0): (1, True, True, 3),              # the middle block stands alone
    (32, 32, 100, 0): (2, False, True, 1), (65, 8, 130, 0): (2, False, True, 2), (65, 8, 130, 37): (2, False, True, 2),
    (171, 3, 130, 0): (2, False, False, 2),
    (16, 32, 130, 0): (2, True, True, 2),
    (16, 32, 300, 0): (2, True, True, 3),
}
# hi + lo operands always run NQ = 1; (32, 32, 100, 0) adds no branch there and is dropped.  (paired, nt) of the large shapes:
PREFILL_SPLIT_DROPPED = [(32, 32, 100, 0)]
PREFILL_SPLIT_LARGE = {(16, 32, 100, 0): (True, 2), (8, 32, 150, 0): (True, 3), (65, 8, 130, 37): (False, 3), (65, 8, 130, 0): (False, 3),
                       (171, 3, 130, 0): (False, 3), (16, 32, 130, 0): (True, 3), (16, 32, 300, 0): (False, 5)}
PREFILL_ALIBI = [(1, 3, 130, 0), (16, 32, 100, 0), (65, 8, 130, 0)]          # one small, one paired, one NQ = 2 (bf16 operands)


def prefill_case_id(shape, mode, alibi):
    batch, nh, s, past = shape
    r = prefill_rule(batch, nh, s, mode == "split")
    inst = f"<{int(mode == 'split')},{r.nq},{int(mode != 'lse')},{int(alibi)}>"
    return f"{mode}{'_alibi' if alibi else ''}-{batch}x{nh}x{s}p{past}-{inst}-{'paired' if r.paired else 'single'}-nt{r.nt}-{'xcd' if r.xcd else 'lin'}"


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, past, slopes=None, dtype=torch.float64, visible=None, total=None, bounds=True, want_p=False, budget=25e6, device=None):
    """Causal attention of q [N][S][128] over k / v [N][T][128]: query i sees key j <= past + i (``visible`` [S][T] bool overrides
    that).  ``slopes`` [N] adds slope_n * (j - (total - 1)) to the scaled scores (total = past + S).  Evaluated in ``dtype`` over
    chunks of heads so that no more than ``budget`` scores are alive; ``device``: where the chunks are evaluated (operands and
    results stay on the host).  Returns out [N][S][128], lse [N][S] (natural log), and with ``bounds`` B [N][S][128] and A [N][S];
    with ``want_p`` the probabilities [N][S][T]."""
    N, S, _ = q.shape
    T = k.shape[1]
    total = past + S if total is None else total
    if visible is None:
        visible = torch.arange(T)[None, :] <= past + torch.arange(S)[:, None]
    rel = (torch.arange(T) - (total - 1)).to(dtype)
    if device is not None:
        visible, rel = visible.to(device), rel.to(device)
    out, lse = torch.empty((N, S, HD), dtype=dtype), torch.empty((N, S), dtype=dtype)
    Bb = torch.empty((N, S, HD), dtype=dtype) if bounds else None
    Aa = torch.empty((N, S), dtype=dtype) if bounds else None
    P = torch.empty((N, S, T), dtype=dtype) if want_p else None
    step = max(1, int(budget // (S * T)))
    for n0 in range(0, N, step):
        sl = slice(n0, min(N, n0 + step))
        qc, kc, vc = (t[sl].to(device=device, dtype=dtype) for t in (q, k, v))
        s = torch.matmul(qc, kc.transpose(1, 2)) * SCALE
        bias = None
        if slopes is not None:
            bias = slopes[sl].to(device=device, dtype=dtype)[:, None, None] * rel[None, None, :]
            s = s + bias
        s = s.masked_fill(~visible[None], float("-inf"))
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        p = e / l
        out[sl] = torch.matmul(p, vc)
        lse[sl] = (m + torch.log(l))[..., 0]
        if want_p:
            P[sl] = p
        if bounds:
            Bb[sl] = torch.matmul(p, vc.abs())
            a = torch.matmul(qc.abs(), kc.abs().transpose(1, 2)) * SCALE
            if bias is not None:
                a = a + bias.abs()
            Aa[sl] = a.masked_fill(~visible[None], 0.0).amax(-1)
    return SimpleNamespace(out=out, lse=lse, B=Bb, A=Aa, p=P)


def reference(q, k, v, past, slopes=None):
    """the float64 reference with its bounds, plus torch's float32 result of the same operation on the same operands (for ``c``)"""
    ref = attention(q, k, v, past, slopes)
    t32 = attention(q.float(), k.float(), v.float(), past, None if slopes is None else slopes.float(), dtype=torch.float32, bounds=False)
    ref.out32, ref.lse32 = t32.out, t32.lse
    return ref


FORMAT = {        # kind -> the coefficient of B that comes from the number formats, as a function of A
    "decode": lambda A: 0.0 * A,
    "decode_split": lambda A: 0.0 * A,
    "bf16": lambda A: 2.0 ** -16 + 0.0 * A,
    "split": lambda A: 2.0 ** -16 * (2.0 + 2.0 * A),
    "lse": lambda A: 2.0 ** -8 + 0.0 * A,
}
TWO_PLANES = ("decode_split", "split")


def out_tolerance(kind, ref):
    """(atol per element as numpy, r of torch fp32): u + (format coefficient + c 2^-24 (1 + 2A)) B"""
    A = ref.A[..., None]
    fp32_bound = (1.0 + 2.0 * A) * ref.B
    atol32, r = tol(f"{kind} out", ref.out32, ref.out, fp32_bound)
    u = 2.0 ** -16 * ref.out.abs().numpy() if kind in TWO_PLANES else bf16_ulp(ref.out)
    return u + (FORMAT[kind](A) * ref.B).numpy() + atol32, r


def lse_tolerance(ref):
    bound = 1.0 + ref.lse.abs() + ref.A
    return tol("lse", ref.lse32, ref.lse, bound)


def check_out(name, kind, got, ref, sel=None):
    """``got`` [N][S][128] (float64: the plane, or hi + lo) against the reference under the bound of ``kind``; ``sel`` restricts the
    comparison to some heads (a boolean [N])"""
    atol, r = out_tolerance(kind, ref)
    want = ref.out
    if sel is not None:
        got, want, atol = got[sel], want[sel], atol[sel.numpy()]
    return check_frac(name, got, want, atol, r)


def check_lse(name, got, ref):
    atol, r = lse_tolerance(ref)
    return check_frac(name, got, ref.lse, atol, r)


def to_rows(x, batch, nh):
    """[N][S][128] -> the kernels' output layout [batch * S][nh * 128]"""
    S = x.shape[1]
    return x.view(batch, nh, S, HD).permute(0, 2, 1, 3).reshape(batch * S, nh * HD)


def from_rows(x, batch, nh):
    S = x.shape[0] // batch
    return x.view(batch, S, nh, HD).permute(0, 2, 1, 3).reshape(batch * nh, S, HD)


# ---------------------------------------------------------------------------------------------------------------------
# planted inputs
# ---------------------------------------------------------------------------------------------------------------------
PLANT = 0.6        # k_j += 0.6 q_i: with q, k ~ 1.5 N(0, 1) that key's score rises by 0.6 * 128 * 2.25 / sqrt(128) = 15 -> p ~ 0.9


def prefill_plants(s, past, nq):
    """(visible (query, key) pairs, masked pairs).  Visible: the diagonal key past + i of the first, 16th, 17th and last query of a
    wave's set (every set boundary of the first block) and of the ragged last block; keys 63 and 64, key 0, the first key of the
    ragged tile, the last key.  Masked: the first masked key past + i + 1 of a few queries -- it must not show."""
    total = past + s
    bq = 64 * nq
    last0 = bq * ((s - 1) // bq)
    diag = {0, 15, 16, 31, 32, 47, 48, 63, 64, 127, 128} | {last0, last0 + 15, last0 + 16, s - 1} | {64 * ((s - 1) // 64)}
    pairs = [(i, past + i) for i in sorted(diag) if 0 <= i < s]
    for j in (0, 63, 64, 64 * (total // 64), total - 1):
        if 0 <= j < total:
            i = min(s - 1, max(j - past, 0) + 3)                      # a query a little below the diagonal of key j
            if (i, j) not in pairs:
                pairs.append((i, j))
    masked = [(i, past + i + 1) for i in sorted({0, 1, 15, 16, 62, 63, last0, s - 2}) if 0 <= i and i + 1 < s]
    return pairs, masked


def decode_plants(total):
    """keys planted for the one query of a decode step: both sides of the 64-key tile, of the 128-key (4 waves) and 256-key (16 waves)
    rounds of loads and of the 8-key V chunk, key 0, the first key of the ragged tile, the last key"""
    keys = {0, 7, 8, 63, 64, 127, 128, 255, 256, 64 * (total // 64), 8 * ((total - 1) // 8), total - 2, total - 1}
    return sorted(j for j in keys if 0 <= j < total)


def prefill_operands(batch, nh, s, past, split):
    """seeded q (x1.5), k (x1.5), v with the planted keys, as planes: dict of q / k / v -> (hi, lo or None), [N][S or total][128]"""
    g = gen(batch, nh, s, past, 77)
    N, total = batch * nh, past + s
    q = torch.randn(N, s, HD, generator=g) * 1.5
    k = torch.randn(N, total, HD, generator=g) * 1.5
    v = torch.randn(N, total, HD, generator=g)
    nq = prefill_rule(batch, nh, s, False).nq
    vis, masked = prefill_plants(s, past, nq)
    for i, j in vis + masked:
        k[:, j] += PLANT * q[:, i]
    cut = (lambda x: planes(x)) if split else (lambda x: (x.bfloat16(), None))
    return {"q": cut(q), "k": cut(k), "v": cut(v)}


def k_cache(plane, batch, nh, smax):
    """[N][total][128] -> the K cache [batch][nh][smax][128] with every position >= total holding GARBAGE"""
    N, total, _ = plane.shape
    c = garbage((N, smax, HD))
    c[:, :total] = plane
    return c.view(batch, nh, smax, HD)


def vt_cache(plane, batch, nh, smax):
    """[N][total][128] -> the transposed V cache [batch][nh][128][smax], columns >= total GARBAGE"""
    N, total, _ = plane.shape
    c = garbage((N, HD, smax))
    c[:, :, :total] = plane.transpose(1, 2)
    return c.view(batch, nh, HD, smax)


# ---------------------------------------------------------------------------------------------------------------------
# float32 / bf16-flow emulations of the kernels' arithmetic, and wrong kernels (tests/test_llama_kernel_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def emulate(kind, q, k, v, past, slopes=None, visible=None, total=None, quarter_max=False):
    """The kernels' number formats on the CPU: float32 scores and probabilities; the probabilities enter the second product as
    bf16 hi + lo (bf16 / split), rounded to bf16 once (lse) or as they are (decode); exact accumulation; the row sum over the
    unrounded probabilities; one rounding of the output to its planes.  ``visible`` / ``total`` state a wrong mask;
    ``quarter_max`` takes the running maximum over the first quarter of the visible keys only (the folded-away v_max) and rounds the
    probabilities, renormalised against it, to one bf16 plane."""
    N, S, _ = q.shape
    T = k.shape[1]
    total = past + S if total is None else total
    if visible is None:
        visible = torch.arange(T)[None, :] <= past + torch.arange(S)[:, None]
    q32, k32 = q.float(), k.float()
    s = torch.matmul(q32, k32.transpose(1, 2)) * np.float32(SCALE)
    if slopes is not None:
        s = s + slopes.float()[:, None, None] * (torch.arange(T) - (total - 1)).float()[None, None, :]
    s = s.masked_fill(~visible[None], float("-inf"))
    if quarter_max:
        nvis = visible.sum(-1, keepdim=True)
        first = visible & (torch.cumsum(visible.int(), -1) <= torch.clamp(nvis // 4, min=1))
        m = s.masked_fill(~first[None], float("-inf")).amax(-1, keepdim=True)
    else:
        m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.double().sum(-1, keepdim=True)
    if quarter_max:                                      # ... with the probabilities rounded to bf16 once
        e = e.bfloat16().double()
    elif kind in ("bf16", "split"):
        hi, lo = planes(e)
        e = hi.double() + lo.double()
    elif kind == "lse":
        e = e.bfloat16().double()
    else:
        e = e.double()
    o = (torch.matmul(e, v.double()) / l).float()
    lse = (m.double() + torch.log(l))[..., 0].float()
    if kind in TWO_PLANES:
        hi, lo = planes(o)
        return hi.double() + lo.double(), lse
    return o.bfloat16().double(), lse


# ---------------------------------------------------------------------------------------------------------------------
# RoPE, RMSNorm, embedding
# ---------------------------------------------------------------------------------------------------------------------
def rope_tables(max_pos):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, HD, 2, dtype=torch.float32) / HD))
    f = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return f.cos().contiguous(), f.sin().contiguous()


def rope(x, c, s, dtype=torch.float64):
    """half-split rotation of x [..., 128] with c, s [..., 64] (the GIVEN table rows): x * cos + rotate_half(x) * sin.  In float32
    this is the kernel's own expression, rounding for rounding: q1 * c + (-q2) * s | q2 * c + q1 * s."""
    x, c, s = x.to(dtype), c.to(dtype), s.to(dtype)
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat((x1 * c + (-x2) * s, x2 * c + x1 * s), dim=-1)


def rope_bound(x, c, s):
    """|x1 c| + |x2 s| per element: what the 4 * 2^-24 fp32 term of the RoPE tolerance multiplies"""
    x, c, s = x.double().abs(), c.double().abs(), s.double().abs()
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat((x1 * c + x2 * s, x2 * c + x1 * s), dim=-1)


def rmsnorm(x, w, eps, dtype=torch.float64):
    x, w = x.to(dtype), w.to(dtype)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return w * (x * rstd), rstd


def embed(ids, table):
    vocab = table.shape[0]
    return table[ids.clamp(0, vocab - 1)].float()
