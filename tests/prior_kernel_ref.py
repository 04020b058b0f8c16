"""References, inputs, plants and bounds for the kernel-level tests of the Jukebox prior's kernels of csrc/prior.hip
(prior_attn16_kernel<NK32>, layernorm_split_kernel / layernorm_split8_kernel, prior_head_kernel, prior_embed_kernel, ln_row_pred_kernel,
pool_window_kernel, pool_mean_kernel, zero_pad16_kernel).  A plain module: tests/test_prior_kernels_gpu.py runs the kernels against it,
tests/test_prior_kernel_ref_cpu.py proves on the CPU that its bounds reject wrong kernels and accept the documented arithmetic.

Layout used throughout: q, k, v [n][heads][t][hd] fp32 are the operand VALUES exactly as the kernel reads them from qkv [n * t][ldq]
(q | k | v column blocks of n_state = heads * hd each, head h at columns h * hd ..); the kernel's own fp16 hi / lo split is part of
what is tested.  The visible sets are stated here per (query i, key j) with b = i // block_ctx, independently of the oracle:

    pattern 1 (block)        j in block b and j <= i
    pattern 2 (transposed)   j % block_ctx == i % block_ctx and j // block_ctx <= b
    pattern 3 (previous)     j in block b - 1; block 0 sees nothing and its output is exact zeros in both planes

The number format.  A value x is carried as fp16 planes hi = fp16(x), lo = fp16(x - hi).  While lo is a NORMAL fp16 the pair is
within 2^-22 |x| of x ("22 bits").  lo is subnormal as soon as |x - hi| < 2^-14, which holds for every |x| < 2^-3: there its spacing
is 2^-24 and the pair carries an ABSOLUTE error of up to 2^-25 whatever |x| is.  Both cases: |x - hi - lo| <= 2^-22 |x| + 2^-25.
Softmax probabilities are almost always below 2^-3, so the floor is the common case for p, and for q, k, v at realistic scales.

Bound of the attention output, per element; over the visible keys j of a query, with s = 1 / sqrt(hd), p the exact probabilities,
B = sum_j p_j |v_jd| and A = max_j s sum_d |q_d| |k_jd|:

  * scores: s sum_d (qh kh + qh kl + ql kh) leaves out ql kl (<= 2^-22 |q||k|) and inherits the split errors of q and k:
    |ds_j| <= 3 * 2^-22 s sum_d |q_d||k_jd|  +  2^-25 s sum_d (|q_d| + |k_jd|)  <=  3 * 2^-22 A + 2^-25 s max_j sum_d (|q_d| + |k_jd|)
    (products of two error terms are of second order).  A score error moves p_j by p_j ds_j and the normaliser by at most max ds:
    the output moves by at most 2 max|ds| B.
  * P V: sum_j (ph vh + ph vl + pl vh) leaves out pl vl and inherits the split errors of p (<= 2^-22 p + 2^-25) and v:
    <= 3 * 2^-22 B + 2^-25 (sum_j p_j + sum_j |v_jd|) = 3 * 2^-22 B + 2^-25 (1 + sum_visible |v_jd|)
  * the output planes: 2^-22 |o| + 2^-25 <= 2^-22 B + 2^-25.

    tol = c * ( 2^-22 (1 + 2A) B + F )
    F   = 2^-25 (2 + sum_visible |v_jd|)  +  2 B * 2^-25 s max_j sum_d (|q_d| + |k_jd|)

F collects every 2^-25 term above: it is the floor of subnormal lo planes in q, k, p, v and the output.  The integer factors
(3 + 1 on B, 2 * 3 on A B) and the fp32 roundings of the accumulations, of expf and of the normalisation (a few 2^-24) sit in
c = max(4, 4 r): kernel_util.tol's constant max(16, 4 r) expressed in the 2^-22 unit, r = the worst ratio err / (2^-22 (1 + 2A) B + F)
of ``emulate`` -- a CPU emulation of the documented arithmetic (fp16 hi / lo operands, three products per pair, fp32 softmax, the
output split again) -- on the same inputs, never taken from the kernel.  Where no key is visible the tolerance is 0.

Plants (unit scale only: at the small scale an aligned key would need |k| ~ 50 to reach that score): k_j += ALPHA(hd) q_i lifts the
score of key j for query i by about 12 and v_j = +-4: a masked plant that is admitted, or a visible one that is dropped, moves the
output by O(|v|).  ``attn_plants`` lists them: the first and last visible key, keys 63 and 64 of a 128-key range; masked: the next
key / block, the own block and block b - 2 of pattern 3, the same position in the other clip and in the neighbouring head.

Row kernels: LayerNorm planes against float64 layer_norm under the fp32 LayerNorm bound of tests/test_mpt_kernels_gpu.py
(B = rstd |gamma| (|x| + mean|x|) + |beta|, c from torch's own float32 result, kernel_util.tol) plus 2^-22 |y| + 2^-25 for the planes;
pool_window / pool_mean under the sequential fp32 sum bound (L + 2) 2^-24 sum|h| / L; everything else is bit-exact.

Measured on an MI355X (kernel = its worst |error| as a fraction of tol, c = 4 throughout; r = the emulation's worst ratio in the c = 1
bound, so the emulation itself sits at r / 4 of tol), per case and pattern 1 | 2 | 3:

    case          r (emulation)               kernel, fp16 lo plane         kernel, lo8 (tol + e4m3 term)
    a             0.415  0.418  0.177         0.104   0.104   0.0399        0.416  0.480  0.316
    b             0.557  0.520  0.135         0.139   0.130   0.0443
    c             0.437  0.301  0.308         0.109   0.0753  0.0770
    d             0.589  0.485  0.259         0.147   0.121   0.0782
    e             0.481  0.376  0.319         0.120   0.0939  0.0798        0.506  0.385  0.253
    f             0.322  0.441  0.138         0.0804  0.110   0.0302
    g             0.244  0.219  0.283         0.0610  0.0457  0.0708        0.488  0.411  0.604
    a, small      0.807  0.928  0.436         0.202   0.220   0.109
    e, small      0.943  0.863  0.795         0.236   0.216   0.199

The kernels sit where the emulation sits (r / 4, mostly to three digits): they compute the documented arithmetic, at every
instantiation, numbering and chunk count of the table, and nothing had to be changed in csrc/prior.hip.  Against the same bound WITHOUT
its floor F the emulation -- the format itself -- is at up to 362 x (unit scale, case a pattern 2) and 1.85e5 x (case e small, pattern 1):
a purely relative 2^-22 bound cannot be met by fp16 hi / lo planes, which is what include/llark_hip.h now says.

LayerNorm planes, worst over the widths and row counts of the tables (torch = its float32 CPU result, in 2^-24 B):

    data                 torch     kernel, fraction of tol: 8-column form   4-column form   lo8 (either form; + e4m3 term)
    2 randn + 0.5        3.5       0.22                                     0.25            0.85
    mean 300, std 0.01   1.7       0.064                                    0.060           0.060
    a constant row       3.0       0.22                                     0.24            0.85

(the lo8 figures are the e4m3 rounding itself: 3 mantissa bits round by up to 2^-4 of the residual, which is that term.)
ln_row_pred's mean: at most 0.066 of its tolerance (torch 1.05 x 2^-24 B); its scale, prior_embed, prior_head and zero_pad16 are exact.
"""
import functools
import math
from types import SimpleNamespace

import torch

from conftest import report_close
from kernel_util import check_frac, gen, tol

U22, U25 = 2.0 ** -22, 2.0 ** -25
PATTERNS = (1, 2, 3)

# case -> (n, t, heads, hd, blocks)
ATTN_CASES = {
    "a": (2, 512, 2, 24, 8),          # NK32 = 1; pattern 2 with 8 queries / keys; clip isolation
    "b": (1, 170, 3, 34, 5),          # NK32 = 2; block_ctx % 8 != 0; ragged 34-row tiles; 3 heads
    "c": (2, 512, 1, 66, 64),         # NK32 = 3; pattern 2: one full 64-key chunk, XCD numbering, grid.x = 8
    "d": (1, 2048, 2, 128, 128),      # NK32 = 4; pattern 2: two chunks, 128 keys, coff = 64, XCD numbering
    "e": (1, 768, 2, 150, 128),       # NK32 = 5; two chunks with the fallback numbering
    "f": (2, 128, 1, 160, 2),         # largest head_dim; pattern 3 with one live block
    "g": (1, 64, 1, 2, 64),           # smallest head_dim; one-token blocks
}
SCALES = {"unit": (1.5, 1.0), "small": (0.05, 0.02)}          # (q and k, v)
ATTN_RUNS = [(c, "unit") for c in ATTN_CASES] + [("a", "small"), ("e", "small")]
LO8_CASES = ("a", "e", "g")


def round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------
# launcher rule (csrc/prior.hip: prior_attn_impl and the head of prior_attn16_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def attn_rule(t, heads, hd, blocks, pattern):
    """what llark_prior_attn picks: the instantiation NK32, queries and (most) keys per workgroup, query chunks of the transposed
    pattern, grid.x and whether the transposed pattern numbers its workgroups XCD-wise ("xcd") or linearly ("linear")"""
    bc = t // blocks
    qc = min(blocks, 64)
    chunks = blocks // qc if pattern == 2 else 1
    nq, nkeys = (qc, chunks * qc) if pattern == 2 else (bc, bc)
    numbering = ("xcd" if bc % 8 == 0 else "linear") if pattern == 2 else None
    return SimpleNamespace(nk32=-(-hd // 32), block_ctx=bc, nq=nq, nkeys=nkeys, chunks=chunks, numbering=numbering,
                           grid_x=bc * chunks if pattern == 2 else blocks)


def attn_refused(t, n_state, heads, blocks, pattern, ldq, ldo):
    """the launcher's refusals, restated"""
    if heads <= 0 or blocks <= 0 or n_state % heads or t % blocks or pattern not in PATTERNS:
        return True
    hd, bc = n_state // heads, t // blocks
    return hd > 160 or bc > 64 or ldq < 3 * n_state or ldo < n_state or blocks > 128 or blocks % min(blocks, 64) != 0 or \
        hd % 2 != 0 or ldq % 2 != 0 or ldo % 2 != 0


# name -> (t, n_state, heads, blocks, pattern, ldq, ldo): each is refused before anything is launched
ATTN_REFUSALS = {
    "hd = 162": (512, 324, 2, 8, 1, 978, 326), "block_ctx = 65": (520, 48, 2, 8, 1, 150, 50), "blocks = 96": (768, 48, 2, 96, 1, 150, 50),
    "odd hd": (512, 46, 2, 8, 1, 144, 48), "odd ldq": (512, 48, 2, 8, 1, 151, 50), "odd ldo": (512, 48, 2, 8, 1, 150, 51),
    "ldq < 3 n_state": (512, 48, 2, 8, 1, 142, 50), "pattern 0": (512, 48, 2, 8, 0, 150, 50), "pattern 4": (512, 48, 2, 8, 4, 150, 50),
    "n_state % heads": (512, 50, 4, 8, 1, 156, 52), "t % blocks": (510, 48, 2, 8, 1, 150, 50),
}


def visible(pattern, t, bc):
    """[t][t] bool: query i sees key j"""
    i, j = torch.arange(t)[:, None], torch.arange(t)[None, :]
    if pattern == 1:
        return (i // bc == j // bc) & (j <= i)
    if pattern == 2:
        return (i % bc == j % bc) & (j // bc <= i // bc)
    if pattern == 3:
        return j // bc == i // bc - 1
    raise ValueError(pattern)


# ---------------------------------------------------------------------------------------------------------------------
# plants and inputs
# ---------------------------------------------------------------------------------------------------------------------
def alpha(hd):
    """k_j += alpha q_i lifts q_i . k_j / sqrt(hd) by alpha |q_i|^2 / sqrt(hd) ~ alpha * 2.25 hd / sqrt(hd) = 12 at q ~ 1.5 N(0, 1)"""
    return 12.0 / (2.25 * math.sqrt(hd))


def attn_plants(pattern, n, t, heads, blocks):
    """list of plants: kind "vis" / "masked", the query (qc, qh, i) and the key row (kc, kh, j) that is aligned to it.  The queries sit
    in the LAST clip and head, so the other clip / neighbouring head plants test rows in front of them."""
    bc = t // blocks
    c0, h0, bl = n - 1, heads - 1, blocks - 1
    out, used = [], set()

    def add(kind, i, j, kc=c0, kh=h0, why=""):
        if (kc, kh, j) in used or not (0 <= j < t):
            return
        used.add((kc, kh, j))
        out.append(SimpleNamespace(kind=kind, qc=c0, qh=h0, i=i, kc=kc, kh=kh, j=j, why=why))

    if pattern == 1:
        i = bl * bc + bc - 1
        add("vis", i, bl * bc, why="first"), add("vis", i, i, why="last")
        i2 = max(bc - 2, 0)
        add("masked", i2, i2 + 1, why="next key")
        last = i
    elif pattern == 2:
        o = bc - 1
        i = bl * bc + o
        add("vis", i, o, why="first"), add("vis", i, i, why="last")
        if blocks == 128:
            add("vis", i, 63 * bc + o, why="key 63"), add("vis", i, 64 * bc + o, why="key 64")
        i2 = (blocks // 2 - 1) * bc
        add("masked", i2, i2 + bc, why="next block")
        last = i
    else:
        i = bl * bc + min(1, bc - 1)
        add("vis", i, (bl - 1) * bc, why="first"), add("vis", i, bl * bc - 1, why="last")
        add("masked", i, i, why="own block")
        if bl >= 2:
            add("masked", i, (bl - 2) * bc + bc - 1, why="block b - 2")
        last = bl * bc - 1
    if n == 2:
        add("masked", i, last, kc=1 - c0, why="other clip")
    if heads >= 2:
        add("masked", i, last, kh=h0 - 1, why="other head")
    return out


def attn_inputs(case, pattern, scale="unit"):
    n, t, heads, hd, blocks = ATTN_CASES[case]
    sqk, sv = SCALES[scale]
    g = gen(ord(case), pattern, len(scale))
    q = torch.randn(n, heads, t, hd, generator=g) * sqk
    k = torch.randn(n, heads, t, hd, generator=g) * sqk
    v = torch.randn(n, heads, t, hd, generator=g) * sv
    plants = attn_plants(pattern, n, t, heads, blocks) if scale == "unit" else []
    for x, p in enumerate(plants):
        k[p.kc, p.kh, p.j] += alpha(hd) * q[p.qc, p.qh, p.i]
        v[p.kc, p.kh, p.j] = torch.where(torch.arange(hd) % (x + 2) == 0, 4.0, -4.0)          # a row of its own per plant
    return SimpleNamespace(case=case, pattern=pattern, scale=scale, n=n, t=t, heads=heads, hd=hd, blocks=blocks, bc=t // blocks,
                           q=q, k=k, v=v, plants=plants)


def to_rows(x):
    """[n][heads][t][hd] -> the kernels' row layout [n * t][heads * hd]"""
    n, heads, t, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * t, heads * hd)


def from_rows(x, n, heads):
    rows, S = x.shape
    return x.view(n, rows // n, heads, S // heads).permute(0, 2, 1, 3)


def qkv_rows(inp, ldq):
    """qkv [n * t][ldq] fp32 with NaN in the pad columns"""
    S = inp.heads * inp.hd
    buf = torch.full((inp.n * inp.t, ldq), float("nan"), dtype=torch.float32)
    buf[:, :S], buf[:, S:2 * S], buf[:, 2 * S:3 * S] = to_rows(inp.q), to_rows(inp.k), to_rows(inp.v)
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference with its bound, and the emulation of the documented arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def dense(q, k, v, vis, bounds=True):
    """dense masked softmax attention in float64 over [t][t] per (clip, head): out and (with ``bounds``) the c = 1 bound
    2^-22 (1 + 2A) B + F per element, 0 where the query sees no key"""
    n, heads, t, hd = q.shape
    s_ = 1.0 / math.sqrt(hd)
    live = vis.any(-1)
    out = torch.zeros((n, heads, t, hd), dtype=torch.float64)
    bound = torch.zeros_like(out) if bounds else None
    rel = torch.zeros_like(out) if bounds else None          # the same without the floor F: a purely relative 2^-22 bound
    visd = vis.double()
    for c in range(n):
        for h in range(heads):
            qc, kc, vc = q[c, h].double(), k[c, h].double(), v[c, h].double()
            s = (qc @ kc.T * s_).masked_fill(~vis, float("-inf"))
            m = torch.where(live, s.amax(-1), s.new_zeros(())).unsqueeze(-1)
            e = torch.exp(s - m)
            p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
            out[c, h] = p @ vc
            if bounds:
                B = p @ vc.abs()
                A = ((qc.abs() @ kc.abs().T) * s_ * visd).amax(-1, keepdim=True)
                sumv = visd @ vc.abs()
                qk1 = (qc.abs().sum(-1) + (visd * kc.abs().sum(-1)[None, :]).amax(-1)).unsqueeze(-1)
                rel[c, h] = U22 * (1.0 + 2.0 * A) * B * live.unsqueeze(-1)
                bound[c, h] = rel[c, h] + (U25 * (2.0 + sumv) + 2.0 * B * U25 * s_ * qk1) * live.unsqueeze(-1)
    return out, bound, rel


def split16(x32):
    """fp32 -> the values of the fp16 hi plane and of the fp16 plane of the rounding residual, as float64"""
    hi = x32.half()
    return hi.double(), (x32 - hi.float()).half().double()


def emulate(q, k, v, vis, scale=None, drop_qk=False, drop_pv=False, drop_out_lo=False):
    """The documented arithmetic on the CPU: q, k, v as fp16 hi + lo, three products per pair (lo.lo dropped) accumulated exactly and
    rounded to fp32 once, the fp32 scale (hd^-1/4)^2, an fp32 softmax, p as hi + lo, the output split again.  ``scale`` overrides
    1 / sqrt(hd); drop_qk / drop_pv leave out the lo.hi pass of a product; drop_out_lo returns the hi plane alone."""
    n, heads, t, hd = q.shape
    sc = 1.0 / math.sqrt(math.sqrt(hd))
    s32 = torch.tensor(sc * sc if scale is None else scale, dtype=torch.float32)
    live = vis.any(-1)
    out = torch.zeros((n, heads, t, hd), dtype=torch.float64)
    for c in range(n):
        for h in range(heads):
            (qh, ql), (kh, kl), (vh, vl) = split16(q[c, h]), split16(k[c, h]), split16(v[c, h])
            acc = qh @ kh.T + qh @ kl.T
            if not drop_qk:
                acc = acc + ql @ kh.T
            s = (acc.float() * s32).masked_fill(~vis, float("-inf"))
            m = torch.where(live, s.amax(-1), s.new_zeros(())).unsqueeze(-1)
            e = torch.exp(s - m)
            l = e.sum(-1, keepdim=True)
            p = e * torch.where(l > 0, 1.0 / l, l.new_zeros(()))
            ph, pl = split16(p)
            o = ph @ vh + ph @ vl
            if not drop_pv:
                o = o + pl @ vh
            oh, ol = split16(o.float())
            out[c, h] = oh if drop_out_lo else oh + ol
    return out


def make_reference(inp):
    vis = visible(inp.pattern, inp.t, inp.bc)
    out, bound, rel = dense(inp.q, inp.k, inp.v, vis)
    emu = emulate(inp.q, inp.k, inp.v, vis)
    err = (emu - out).abs()
    pos = bound > 0
    assert bool((err[~pos] == 0).all()), "the emulation is off where no key is visible"
    r = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    c = max(4.0, 4.0 * r)
    r_rel = float((err[pos] / rel[pos]).max()) if pos.any() else 0.0          # what the emulation needs of a bound without F
    return SimpleNamespace(inp=inp, vis=vis, out=out, bound=bound, r=r, r_rel=r_rel, c=c, tol=(c * bound).numpy(), emu=emu)


@functools.lru_cache(maxsize=None)
def attn_reference(case, pattern, scale="unit"):
    """computed once per (case, pattern, scale) and shared; nobody writes to it"""
    return make_reference(attn_inputs(case, pattern, scale))


def check_attn(name, got, ref, extra=None):
    """``got`` [n][heads][t][hd] float64 (hi + lo) against the reference under tol = c (2^-22 (1 + 2A) B + F) (+ ``extra``, numpy, per
    element); prints the worst fraction of the tolerance next to the emulation's r and returns that fraction"""
    got = got.detach().cpu().double()
    atol = ref.tol if extra is None else ref.tol + extra
    err = (got - ref.out).abs().numpy()
    pos = atol > 0
    frac = float((err[pos] / atol[pos]).max()) if pos.any() else 0.0
    print(f"[ratio] {name}: kernel {frac:.3g} of its tolerance (c = {ref.c:.3g}), emulation r = {ref.r:.3g} x the c = 1 bound")
    report_close(name, got.numpy(), ref.out.numpy(), atol)
    return frac


# ---------------------------------------------------------------------------------------------------------------------
# lo8: the e4m3 low plane in MFMA slot order (include/llark_hip.h, llark_gemm16_lo8)
# ---------------------------------------------------------------------------------------------------------------------
def lo8_pos(k):
    """byte offset of element k of a row: 64-element blocks, element k of a block at 32 (k / 8 % 2) + 8 (k / 16 % 4) + k % 8"""
    k = torch.as_tensor(k)
    r = k % 64
    return (k - r) + 32 * ((r // 8) % 2) + 8 * ((r // 16) % 4) + r % 8


def lo8_written(rows, ldo8, width):
    m = torch.zeros((rows, ldo8), dtype=torch.bool)
    m[:, lo8_pos(torch.arange(width))] = True
    return m


def e4m3_term(ref64, hi64, sa):
    """what an e4m3 plane (3 mantissa bits, subnormal step 2^-9, scaled by 2^sa) adds to the error of hi + lo8"""
    return (2.0 ** -4 * (ref64 - hi64).abs() + 2.0 ** -10 * 2.0 ** -sa).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm -> planes
# ---------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
LN8_WIDTHS = [8, 512, 520, 2048, 2056, 4800, 5128, 8192]                      # 8 columns per lane: NG = 1 | 4 | 10 | 16, both sides
LN4_WIDTHS = [4, 252, 260, 1020, 1028, 4092, 4100, 4860, 4868, 8188]          # 4 columns per lane: NV = 1 | 4 | 16 | 19 | 32
LN_FORCED4 = [512, 5128]                                                      # width % 8 == 0 with ldo % 8 == 4: the 4-column form
LN_ROWS = [1, 5, 9]
LN_DATA = ["randn", "offset", "const"]
LN_LO8_WIDTHS = [8, 520, 4800, 5128, 8192, 4, 260, 4100, 4868, 8188]


def ln_rule(width, ldx, ldo):
    """("8", NG) / ("4", NV): the kernel form and instantiation layernorm_split_impl picks for 16-byte aligned pointers; None: refused"""
    if width <= 0 or width % 4 or ldx % 4 or ldo % 4 or ldo < width or ldx < width:
        return None
    if width % 8 == 0 and ldx % 8 == 0 and ldo % 8 == 0:
        w8 = width // 8
        return next((("8", ng) for ng, cap in ((1, 64), (4, 256), (10, 640), (16, 1024)) if w8 <= cap), None)
    w4 = width // 4
    return next((("4", nv) for nv, cap in ((1, 64), (4, 256), (16, 1024), (19, 1216), (32, 2048)) if w4 <= cap), None)


def ln_lds(width, forced4=False):
    """(ldx, ldo) with pad columns that keep the row kernels on the form the width belongs to"""
    if width % 8 == 0 and not forced4:
        return width + 8, width + 16
    return width + 4, width + 4 if width % 8 else width + 12


def head_ng(width):
    return next(ng for ng, cap in ((1, 64), (4, 256), (10, 640), (16, 1024)) if width // 8 <= cap)


def ln_inputs(rows, width, data):
    g = gen(rows, width, LN_DATA.index(data))
    if data == "randn":
        x = 2.0 * torch.randn(rows, width, generator=g) + 0.5
    elif data == "offset":
        x = 300.0 + 0.01 * torch.randn(rows, width, generator=g)
    else:
        x = 2.0 * torch.randn(rows, width, generator=g) + 0.5
        x[rows // 2] = 0.7
    gamma = 1.0 + 0.2 * torch.randn(width, generator=g)
    beta = 0.1 * torch.randn(width, generator=g)
    return x, gamma, beta


def ln_reference(x, gamma, beta):
    """(float64 layer_norm, per-element tolerance as numpy, r of torch's float32 layer_norm): the fp32 LayerNorm bound
    c 2^-24 rstd |gamma| (|x| + mean|x|) + |beta|, plus 2^-22 |y| + 2^-25 for the fp16 hi + lo planes"""
    width = x.shape[1]
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    ref = torch.nn.functional.layer_norm(x64, (width,), g64, b64, LN_EPS)
    rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + LN_EPS)
    bound = rstd * g64.abs() * (x64.abs() + x64.abs().mean(-1, keepdim=True)) + b64.abs()
    t32 = torch.nn.functional.layer_norm(x, (width,), gamma, beta, LN_EPS)
    atol, r = tol("layer_norm", t32, ref, bound)
    return ref, atol + (U22 * ref.abs() + U25).numpy(), r


# ---------------------------------------------------------------------------------------------------------------------
# ln_row_pred
# ---------------------------------------------------------------------------------------------------------------------
PRED_WIDTHS = [4, 260, 4800, 8192]
PRED_ROWS = [1, 5]
PRED_MARGIN = 0.02


def pred_reference(x):
    """float64 (mean, rstd, log2 rstd) of the rows of x"""
    x64 = x.double()
    mean = x64.mean(-1)
    rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + LN_EPS)
    return mean, rstd, torch.log2(rstd)


def pred_margin(x):
    """the smallest distance of frac(log2 rstd) from 0.5 over the rows: how far every row is from the rounding edge of the scale"""
    l2 = pred_reference(x)[2]
    return float(((l2 - torch.floor(l2)) - 0.5).abs().min())


def pred_inputs(rows, width):
    """rows of different level and spread (std 0.05 .. 20); the first seed whose rows all keep PRED_MARGIN from the rounding edge of
    2^round(log2 rstd), found on the float64 reference"""
    for seed in range(200):
        g = gen(rows, width, seed, 31)
        spread = torch.exp2(torch.rand(rows, 1, generator=g) * 8.6 - 4.3)
        x = torch.randn(rows, width, generator=g) * spread + 0.3 * spread * torch.randn(rows, 1, generator=g)
        if pred_margin(x) >= PRED_MARGIN:
            return x
    raise AssertionError("no seed keeps the margin")


# ---------------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------------
POOL_WINDOW_SHAPES = [(2, 70, 192, 34, 2), (1, 9, 300, 1, 9), (2, 64, 1028, 64, 1)]          # (n, t, width, frame_len, frames)
POOL_MEAN_WIDTHS = [192, 300, 1028]


def pool_bound(h64, L):
    """(mean over the first axis of h64 [L][width], tolerance): a sequential fp32 sum of L terms and one division:
    (L + 2) 2^-24 sum|h| / L"""
    return h64.mean(0), ((L + 2) * 2.0 ** -24 * h64.abs().sum(0) / L).numpy()
