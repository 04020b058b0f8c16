"""Reference, inputs and bounds for the kernel-level tests of the flash attention backward of csrc/attn_bwd.hip
(attn_bwd_rowdot_kernel, attn_bwd_dkv_kernel, attn_bwd_dq_kernel behind llark_attn_backward_bf16 and llark_attn_backward_bf16_fused).
A plain module: tests/test_attn_bwd_kernels_gpu.py runs the kernels against it, tests/test_attn_bwd_ref_cpu.py proves on the CPU that
its bounds accept the kernel's arithmetic and reject wrong kernels.  Layout, planted keys, the garbage K-cache rows and the forward
reference are those of tests/llama_kernel_ref.py.

The contract (include/llark_hip.h), as a function of the GIVEN o and lse -- they are operands, not recomputed:

    P_ij = exp(scale q_i.k_j + slope_n (j - (S - 1)) - lse_i) for j <= i, else 0          D_i = sum_d dO_id o_id       dP = dO V^T
    dS = P (dP - D)          dV = P^T dO          dQ = scale dS K          dK = scale dS^T Q          dsum = D

Bounds per output element.  ``A_i`` as in llama_kernel_ref (the largest sum of absolute score terms over the visible keys),
``W_i = 1 + |lse_i| + 2 A_i`` (the relative error of P from fp32 scores and exp2), ``G_ij = sum_d |dO_id| |v_jd| + sum_d |dO_id| |o_id|``
(what the fp32 error of dP_ij - D_i scales with), ``e_ij = W_i |dS_ij| + P_ij G_ij`` (the fp32 error of dS_ij), ``u = 2^-8``:

    dV_jd      u sum_i P_ij |dO_id|                      + c 2^-24 sum_i W_i P_ij |dO_id|          P rounded to bf16 once
    dQ_id      ((1 + u)^2 - 1) scale sum_j |dS_ij| |k_jd|  + c 2^-24 scale sum_j e_ij |k_jd|         P and dS rounded once each
    dK_jd      ((1 + u)^2 - 1) scale sum_i |dS_ij| |q_id|  + c 2^-24 scale sum_i e_ij |q_id|
    dsum_i                                                 c 2^-24 sum_d |dO_id o_id|

plus 2^-24 |ref| for the fp32 store of dq, dk, dv.  ``c = max(16, 4 r)``, ``r`` = the worst ratio of this same function evaluated in torch
float32 on the CPU (``kernel_util.tol``), never of the kernel.  Where a bound is 0 the result must be exact.  At S = 1 (P = 1, D = dP,
dS = 0) the format terms of dq and dk vanish and only the fp32 term P G is left: dP and D are the same 128 products summed in two orders.
"""
from types import SimpleNamespace

import numpy as np
import torch

from kernel_util import EPS24, check_frac, gen, tol
from llama_kernel_ref import HD, SCALE, alibi_slopes, attention, garbage, k_cache  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -8                         # bf16 unit roundoff
PLANT = 0.35                          # k_j += 0.35 q_i: the score rises by 0.35 * 128 * 2.25 / sqrt(128) = 8.9 -> P inside (0, 1) away from the first rows
ON_DEVICE = 8e6                       # cases with more than this many scores (N S^2) evaluate the float64 reference on the device

# (batch, nh, S, smax, alibi) -> (paired, xcd, np, middle tile alone): every path of grid_of / block_to_pair and of the two staging
# paths (csrc/attn_bwd.hip); np = workgroups per head
CASES = {
    (1, 1, 1, 64, False): (False, False, 1, False),           # dS = 0: only the fp32 terms of the bounds are left
    (1, 2, 7, 64, False): (False, False, 1, False),           # one ragged tile
    (1, 3, 64, 64, False): (False, False, 1, False),          # one whole tile, DMA only, smax == S
    (2, 3, 65, 128, False): (False, False, 2, False),         # second tile of one row
    (1, 2, 130, 256, False): (False, False, 3, False),        # three tiles
    (1, 8, 200, 256, False): (False, True, 4, False),         # XCD mapping, unpaired
    (16, 32, 100, 104, False): (True, True, 1, False),        # paired with np = 1: 512 workgroups
    (8, 32, 130, 136, False): (True, True, 2, True),          # paired, odd, ragged
    (8, 32, 256, 256, False): (True, True, 2, False),         # paired, even, all DMA
    (8, 32, 450, 512, False): (True, True, 4, False),         # 1024 workgroups, np = 4
    (171, 12, 100, 128, False): (True, False, 1, False),      # paired on the linear mapping, np = 1
    (171, 6, 130, 136, False): (True, False, 2, True),        # paired, linear, the middle tile alone
    (2, 4, 200, 256, True): (False, True, 4, False),          # ALiBi, unpaired
    (8, 32, 130, 136, True): (True, True, 2, True),           # ALiBi, paired
}
CHAINED = [(1, 2, 130, 256, False), (8, 32, 130, 136, False), (2, 4, 200, 256, True)]      # ragged unpaired, paired odd, ALiBi


def backward_rule(batch, nh, s):
    """the grid llark_attn_backward_bf16 picks (grid_of) and how block_to_pair numbers it: nt tiles of 64 per head, in pairs (the
    p-th longest with the p-th shortest) when the halved grid is 512, 1024 or >= 2048 workgroups; np workgroups per head; ``middle``:
    the middle tile of an odd paired grid stands alone; xcd: whole heads per XCD (batch * nh % 8 == 0), else the linear numbering"""
    nbh = batch * nh
    nt = -(-s // 64)
    wgs = -(-nt // 2) * nbh
    paired = nt >= 2 and (wgs >= 2048 or wgs in (512, 1024))
    np_ = -(-nt // 2) if paired else nt
    return SimpleNamespace(nt=nt, paired=paired, xcd=nbh % 8 == 0, np=np_, middle=paired and nt % 2 == 1, workgroups=np_ * nbh)


def case_id(case):
    batch, nh, s, smax, alibi = case
    r = backward_rule(batch, nh, s)
    return (f"{'alibi-' if alibi else ''}{batch}x{nh}x{s}m{smax}-{'paired' if r.paired else 'single'}-nt{r.nt}-np{r.np}"
            f"{'-middle' if r.middle else ''}-{'xcd' if r.xcd else 'lin'}")


def on_device(case):
    batch, nh, s = case[:3]
    return batch * nh * s * s > ON_DEVICE


# ---------------------------------------------------------------------------------------------------------------------
# the contract reference
# ---------------------------------------------------------------------------------------------------------------------
def _causal(S, T):
    return torch.arange(T)[None, :] <= torch.arange(S)[:, None]


def backward(q, k, v, dO, o, lse, slopes=None, dtype=torch.float64, visible=None, total=None, bounds=True, budget=25e6, device=None):
    """The gradients of causal attention as the header states them, from q, dO, o [N][S][128], k, v [N][T][128] (T = S unless a test
    appends rows), lse [N][S] and ``slopes`` [N]; ``visible`` [S][T] overrides j <= i, ``total`` the S of the ALiBi bias.  Evaluated in
    ``dtype`` over chunks of heads so that no more than ``budget`` scores are alive, on ``device`` (operands and results stay on the
    host).  Returns dq, dk, dv, dsum and, with ``bounds``, the sums the tolerances are made of (module docstring)."""
    N, S, _ = q.shape
    T = k.shape[1]
    total = S if total is None else total
    if visible is None:
        visible = _causal(S, T)
    rel = (torch.arange(T) - (total - 1)).to(dtype)
    if device is not None:
        visible, rel = visible.to(device), rel.to(device)
    names = ["dq", "dk", "dv", "dsum"] + (["dq_u", "dq_e", "dk_u", "dk_e", "dv_u", "dv_e", "dsum_e"] if bounds else [])
    res = {n: torch.empty((N, S if n[1] in "qs" else T) + (() if n.startswith("dsum") else (HD,)), dtype=dtype) for n in names}
    step = max(1, int(budget // (S * T)))
    for n0 in range(0, N, step):
        sl = slice(n0, min(N, n0 + step))
        qc, kc, vc, dOc, oc, lc = (t[sl].to(device=device, dtype=dtype) for t in (q, k, v, dO, o, lse))
        s = torch.matmul(qc, kc.transpose(1, 2)) * SCALE
        bias = None
        if slopes is not None:
            bias = slopes[sl].to(device=device, dtype=dtype)[:, None, None] * rel[None, None, :]
            s = s + bias
        p = torch.exp(s - lc[..., None]).masked_fill(~visible[None], 0.0)
        d = (dOc * oc).sum(-1)
        dp = torch.matmul(dOc, vc.transpose(1, 2))
        ds = p * (dp - d[..., None])
        res["dv"][sl] = torch.matmul(p.transpose(1, 2), dOc)
        res["dq"][sl] = torch.matmul(ds, kc) * SCALE
        res["dk"][sl] = torch.matmul(ds.transpose(1, 2), qc) * SCALE
        res["dsum"][sl] = d
        if not bounds:
            continue
        a = torch.matmul(qc.abs(), kc.abs().transpose(1, 2)) * SCALE
        if bias is not None:
            a = a + bias.abs()
        w = 1.0 + lc.abs() + 2.0 * a.masked_fill(~visible[None], 0.0).amax(-1)
        dabs = (dOc * oc).abs().sum(-1)
        gg = torch.matmul(dOc.abs(), vc.abs().transpose(1, 2)) + (dOc.abs() * oc.abs()).sum(-1)[..., None]
        e = w[..., None] * ds.abs() + p * gg
        res["dv_u"][sl] = torch.matmul(p.transpose(1, 2), dOc.abs())
        res["dv_e"][sl] = torch.matmul((w[..., None] * p).transpose(1, 2), dOc.abs())
        res["dq_u"][sl] = torch.matmul(ds.abs(), kc.abs()) * SCALE
        res["dq_e"][sl] = torch.matmul(e, kc.abs()) * SCALE
        res["dk_u"][sl] = torch.matmul(ds.abs().transpose(1, 2), qc.abs()) * SCALE
        res["dk_e"][sl] = torch.matmul(e.transpose(1, 2), qc.abs()) * SCALE
        res["dsum_e"][sl] = dabs
    return SimpleNamespace(**res)


FORMAT = {"dv": U, "dq": (1.0 + U) ** 2 - 1.0, "dk": (1.0 + U) ** 2 - 1.0, "dsum": 0.0}
OUTPUTS = ("dq", "dk", "dv", "dsum")


def reference(q, k, v, dO, o, lse, slopes=None, device=None):
    """the float64 contract reference with its bound sums, plus the same function in torch float32 on the CPU (for ``c``)"""
    ref = backward(q, k, v, dO, o, lse, slopes, device=device)
    f = lambda t: None if t is None else t.float()
    ref.t32 = backward(f(q), f(k), f(v), f(dO), f(o), f(lse), f(slopes), dtype=torch.float32, bounds=False)
    return ref


def tolerance(name, ref):
    """(atol per element as numpy, r of torch fp32) of output ``name``"""
    want = getattr(ref, name)
    atol32, r = tol(name, getattr(ref.t32, name), want, getattr(ref, name + "_e"))
    if name == "dsum":
        return atol32, r
    atol32 += torch.add(EPS24 * want.abs(), getattr(ref, name + "_u"), alpha=FORMAT[name]).numpy()
    return atol32, r


def check(tag, got, ref, only=OUTPUTS):
    """``got``: dict dq / dk / dv [N][S][128], dsum [N][S] against the reference under the bounds, with the "[ratio]" line of
    ``check_frac`` per output.  Every output is checked before the first failure is raised, so that a failing case prints all ratios."""
    failed = []
    for name in only:
        atol, r = tolerance(name, ref)
        try:
            check_frac(f"{tag} {name}", got[name], getattr(ref, name), atol, r)
        except AssertionError as exc:
            failed.append(str(exc))
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------------------------------
# planted inputs
# ---------------------------------------------------------------------------------------------------------------------
def plants(s):
    """(visible (query, key) pairs, masked pairs).  Visible: the diagonal at the wave and tile edges (queries 0, 15, 16, 31, 32, 47, 48,
    63, 64, S - 1); keys 0, 63, 64, the first key of EVERY 64-key tile -- of the ragged one, and of every tile a paired workgroup takes in
    its second pass -- and key S - 1, each seen from the query 3 below the diagonal.  Masked: the first masked key i + 1 of a few queries."""
    last = 64 * ((s - 1) // 64)
    pairs = [(i, i) for i in sorted({0, 15, 16, 31, 32, 47, 48, 63, 64, s - 1}) if 0 <= i < s]
    for j in sorted({0, 63, 64, s - 1} | set(range(0, s, 64))):
        if 0 <= j < s:
            p = (min(s - 1, j + 3), j)
            if p not in pairs:
                pairs.append(p)
    masked = [(i, i + 1) for i in sorted({0, 1, 15, 16, 62, 63, last, s - 2}) if 0 <= i and i + 1 < s]
    return pairs, masked


def operands(batch, nh, s):
    """seeded bf16 q (x1.5), k (x1.5, with the planted keys), v, dO (x0.1), each [N][S][128]"""
    g = gen(batch, nh, s, 4242)
    N = batch * nh
    q = torch.randn(N, s, HD, generator=g) * 1.5
    k = torch.randn(N, s, HD, generator=g) * 1.5
    v = torch.randn(N, s, HD, generator=g)
    dO = torch.randn(N, s, HD, generator=g) * 0.1
    q = q.bfloat16()
    vis, masked = plants(s)
    for i, j in vis + masked:
        k[:, j] += PLANT * q[:, i].float()
    return {"q": q, "k": k.bfloat16(), "v": v.bfloat16(), "dO": dO.bfloat16()}


def slopes_of(case):
    batch, nh, _, _, alibi = case
    return alibi_slopes(nh).repeat(batch) if alibi else None          # [N], head n = b * nh + h


def forward(ops, slopes, device=None):
    """o (bf16) and lse (fp32) of the float64 forward on these operands: what the isolated tests hand to the backward"""
    fw = attention(ops["q"], ops["k"], ops["v"], 0, slopes, bounds=False, device=device)
    return fw.out.bfloat16(), fw.lse.float()


def planted_p(case, ops, slopes):
    """one line per case: the probabilities of the planted visible pairs in head 0 (a good share should lie well inside (0, 1):
    dS ~ P (1 - P)-like terms vanish at saturation)"""
    vis, _ = plants(case[2])
    p = attention(ops["q"][:1], ops["k"][:1], ops["v"][:1], 0, None if slopes is None else slopes[:1], bounds=False, want_p=True).p
    print(f"[plants] {case_id(case)}: " + " ".join(f"P[{i},{j}]={float(p[0, i, j]):.2f}" for i, j in vis))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's number formats on the CPU, and wrong kernels (tests/test_attn_bwd_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def emulate(q, k, v, dO, o, lse, slopes=None, visible=None, total=None, d_shift=0, dk_scale=True, twice=None, bias_from_query=False):
    """The backward with the kernel's roundings and exact accumulation: float32 exponent x = fma(s, scale log2 e, bias - lse log2 e),
    P = bf16(exp2 x), D and dP in float32, dS = bf16(float(P) (dP - D)) WITHOUT the factor scale, dV = P^T dO, dQ = scale (dS K),
    dK = scale (dS^T Q) rounded to float32.  Wrong kernels: ``visible`` / ``total`` as in ``backward``; ``d_shift``: D taken from row
    i + d_shift; ``dk_scale`` False: dK without its factor; ``twice``: a slice of rows whose dq, dk and dv are accumulated twice;
    ``bias_from_query``: the ALiBi bias slope (key - query)."""
    N, S, _ = q.shape
    T = k.shape[1]
    total = S if total is None else total
    if visible is None:
        visible = _causal(S, T)
    log2e = np.float32(1.4426950408889634)
    scale2 = np.float32(np.float32(SCALE) * log2e)
    qd, kd, vd, dOd = q.double(), k.double(), v.double(), dO.double()
    s32 = torch.matmul(qd, kd.transpose(1, 2)).float()
    add = -(lse.float() * log2e)[..., None]
    if slopes is not None:
        rel = torch.arange(T)[None, :] - (torch.arange(S)[:, None] if bias_from_query else total - 1)
        add = (slopes.float() * log2e)[:, None, None] * rel.float()[None] + add
    x = (s32.double() * float(scale2) + add.double()).float()            # the fma: one rounding
    p = torch.exp2(x.masked_fill(~visible[None], float("-inf"))).bfloat16()
    d = (dOd * o.double()).sum(-1).float()
    dp = torch.matmul(dOd, vd.transpose(1, 2)).float()
    ds = (p.float() * (dp - torch.roll(d, -d_shift, 1)[..., None])).bfloat16()
    scale = np.float32(SCALE)
    dv = torch.matmul(p.double().transpose(1, 2), dOd).float()
    dq = torch.matmul(ds.double(), kd).float() * scale
    dk = torch.matmul(ds.double().transpose(1, 2), qd).float()
    if dk_scale:
        dk = dk * scale
    if twice is not None:
        for t in (dq, dk, dv):
            t[:, twice] *= 2.0
    return {"dq": dq, "dk": dk, "dv": dv, "dsum": d}
