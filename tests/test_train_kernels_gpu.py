"""The Llama training glue and the AdamW step of csrc/train.hip (and the shifted cross-entropy of csrc/llama.hip), one kernel at a
time, against float64 references built on the CPU with plain torch.

Whole-model tests reach these kernels only at hidden 256 (gradients accepted at 3e-2 relative Frobenius error) or use them as the
reference side of a bit-equality test; here every output element is compared with an independent float64 statement of the operation
(float64 autograd of the forward function, torch.softmax, F.cross_entropy, torch.optim.AdamW), at the sizes that select every code
path, with the memory around every output pre-filled with a sentinel and asserted bit-unchanged afterwards, and every input
asserted bit-unchanged.

Tolerances
----------
* exact data movement (the dv third of rope_merge_bwd, dx16 of rmsnorm_bwd_out16, the twins of adamw_twins, zero padding):
  ``torch.equal`` on bits.
* one bf16 output: ``|got - ref64| <= 2**-8 |ref64| + floor`` (``kernel_util.bf16_ulp``), floor = the fp32 bound below of the value
  that is rounded.
* fp32 (and the one double) outputs: ``c * 2**-24 * B``, ``B`` = the float64 sum of the absolute values of the terms entering the
  element, ``c = max(16, 4 * r_torch)``, ``r_torch`` = the worst ratio of torch's own float32 CPU evaluation of the same operation on
  the same inputs (``kernel_util.tol``), measured inside each test, never on the kernel.
* ``under`` (SwiGLU only): where exp(-g) overflows fp32 (g < -88.7) the true sigmoid is below 2**-126 and any fp32 evaluation
  returns 0 for it; the absolute error that allows, 2**-126 times what multiplies the sigmoid, is added to the tolerance and taken off
  the error before the ratio (it is < 1e-30 here and loosens nothing else).

``B`` per output
    swiglu_fwd act            |silu(g) u|
    swiglu_bwd dg             |dact u| sig (1 + |g| (1 - sig))          dgu = [32 dg | 32 du] per 64 columns
    swiglu_bwd du             |dact g| sig
    attn_ds dS                scale |P| (|dP| + sum_{j<=i} |P dP|)
    rope_merge_bwd dq, dk     |d1 c| + |d2 s|   (d1 the gradient of the element itself, d2 of its rotation partner)
    cross_entropy row_loss    |max| + |log sum exp(l - max)| + |l_tgt|;   the mean: the mean of that over the counted rows
    cross_entropy_bwd         (loss_scale / count) (p (|l - max| + 2) + [v == tgt])
    sumsq_f32                 sum x^2
    adamw m                   b1 |m| + (1 - b1) |g|                     (g = the scaled / clipped gradient)
    adamw v                   b2 v + (1 - b2) g^2
    adamw p                   |p| + lr |mhat| / (sqrt(vhat) + eps)
    rmsnorm_bwd dx            rstd (|g| + |xhat| mean|g xhat|) + |dx0|,  g = dy w
    rmsnorm_bwd dw            sum_r |dy xhat| + |dw0|

Measured worst ratios, in units of 2**-24 B, over the cases of this file (torch = its float32 CPU result, kernel = MI355X):

    output                         torch     kernel
    swiglu_fwd act                 3.3       -           (bf16 output: the torch ratio sets its floor, the 2**-8 dominates)
    swiglu_bwd dgu                 13.4      -           (bf16; c = 54 in the worst case)
    attn_ds dS                     4.9       -           (bf16)
    rope_merge_bwd dq, dk          2.0       -           (bf16)
    cross_entropy row_loss         5.6       5.6
    cross_entropy mean loss        0.03      0.35
    cross_entropy_bwd dlogits      10.4      -           (bf16)
    sumsq_f32                      2.5       0.9         (the kernel sums in double)
    adamw / adamw_clip m           2.4       2.3
    adamw / adamw_clip v           4.0       3.8
    adamw p, fp32 parameters       2.9       2.6         (n = 4 194 561 at step 2: torch 20.5, kernel 10.8)
    adamw p, bf16 parameters       2.7       -           (bf16; 21.0 at n = 4 194 561)
    adamw_twins m / v              2.4 / 3.5 2.4 / 4.4
    rmsnorm_bwd dx                 4.6       5.1
    rmsnorm_bwd dw                 4.1       3.7

The AdamW step is compared with the optimizer at the float32-rounded hyperparameters, the operation as the C ABI is called; the
same float64 optimizer with the unrounded Python values (0.999, 1e-8, ...) lies up to 80 x 2**-24 B away at step 1 and 165 at step
2 (printed by every case): that is what passing beta2 as a float costs, and no part of any tolerance.

These tests are why llark_adamw takes its bias corrections 1 - beta**step in double: evaluated in float, as before,
1 - powf(beta2, 2) keeps 15 of its 24 bits, and the fp32 parameters of the step-2 cases come out 51 x 2**-24 B from the reference
(float32 transcription of the former arithmetic on the CPU, against c = 16; step 3 fails the bf16 twins cases at small |p|).

Each test's docstring names the single wrong line it would catch.  Seven of them were confirmed once, off the suite, by mutating
a float32 CPU transcription of the kernel's lines and running this file against it: ``1 - sig`` written as ``sig`` (5 SwiGLU cases
fail), the RoPE backward's sign swapped (4 of 5 cases; S = 1 at position 0 has sin = 0), pos0 ignored (the 3 cases with pos0 != 0),
the AdamW decay dropped (38), eps inside AdamW's square root (50), labels[s] for labels[s + 1] (40), the RMSNorm eps outside the
square root (200); the unmutated transcription passes every case.

``-s`` prints each test's own figures ("[ratio] ...").

``DEV`` / ``_ops`` exist so that the inputs, references, bounds and sentinel checks of this file can be exercised without a GPU by
putting float32 stand-ins in the place of the kernels; the tests themselves always run the HIP library on ``cuda``.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_util import EPS24, assert_untouched as _assert_untouched, bf16_ulp as _bf16_ulp, bf_sentinel as _bf_sentinel, bits as _bits, \
    check as _check, gen as _gen, mask as _mask, nan_buf as _nan_buf, out_slab as _out_slab, slab as _slab, tol as _tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
TINY = 2.0 ** -126
GRID_CAP = 16384 * 256                         # grid_for(): elements one pass of the capped grid covers


def _ops():
    from llark_amd import ops
    return ops


def _err_type():
    from llark_amd import _lib
    return _lib.LlarkHipError


def _to(t):
    return t.to(DEV)


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def _f32(x):
    """the value the C ABI receives for a Python float"""
    return float(np.float32(x))


def _same(name, dev_t, host_t):
    assert torch.equal(_bits(dev_t), _bits(host_t)), f"{name}: an input was modified"


# =====================================================================================================================
# 1. swiglu_fwd / swiglu_bwd
# =====================================================================================================================
SWIGLU_SHAPES = [(1, 32), (3, 96), (5, 352), (37, 11008), (400, 11008)]       # the last: 4 403 200 elements > GRID_CAP
_SW_GATES = [0.0, -0.0, 1e-3, -1e-3, -1.2785, 20.0, -20.0, 100.0, -100.0]    # -1.2785: 1 + g (1 - sig) changes sign
_SW_UPS = [0.0, 1.0, -1.0, 1e3, -1e3]


def _swiglu_cols(inter):
    """column c of act reads gate gu[m][64 (c // 32) + c % 32] and up 32 columns further"""
    c = torch.arange(inter)
    gate = 64 * (c // 32) + c % 32
    return gate, gate + 32


def _swiglu_inputs(rows, inter):
    g = _gen(rows, inter, 1)
    gu = torch.randn(rows, 2 * inter, generator=g) * 3
    dact = torch.randn(rows, inter, generator=g)
    gate, up = _swiglu_cols(inter)
    combos = [(a, b) for a in _SW_GATES for b in _SW_UPS]
    k = min(len(combos), rows * inter)
    pick = [combos[(7 * j) % len(combos)] for j in range(k)]                 # 7 is coprime to 45: a small case still spans the gates
    i = torch.arange(k)
    gu[i // inter, gate[i % inter]] = torch.tensor([a for a, _ in pick])
    gu[i // inter, up[i % inter]] = torch.tensor([b for _, b in pick])
    return gu, dact


def _swiglu_eval(gu, dact, dtype):
    """autograd of silu(gate) * up through explicit index tensors: (act, dgu in the layout of gu)"""
    gate, up = _swiglu_cols(dact.shape[1])
    x = gu.to(dtype).clone().requires_grad_(True)
    act = F.silu(x[:, gate]) * x[:, up]
    act.backward(dact.to(dtype))
    return act.detach(), x.grad


def _swiglu_bounds(gu, dact):
    gate, up = _swiglu_cols(dact.shape[1])
    g, u, d = gu.double()[:, gate], gu.double()[:, up], dact.double()
    sig, nsig = torch.sigmoid(g), torch.sigmoid(-g)
    b_act, u_act = (F.silu(g) * u).abs(), TINY * (1.0 + g.abs()) * u.abs()
    b_dgu, u_dgu = torch.zeros(gu.shape, dtype=torch.float64), torch.zeros(gu.shape, dtype=torch.float64)
    b_dgu[:, gate], b_dgu[:, up] = (d * u).abs() * sig * (1.0 + g.abs() * nsig), (d * g).abs() * sig
    u_dgu[:, gate], u_dgu[:, up] = TINY * (d * u).abs() * (1.0 + g.abs()), TINY * (d * g).abs()
    return b_act, u_act, b_dgu, u_dgu


@pytest.mark.parametrize("rows,inter", SWIGLU_SHAPES, ids=lambda v: str(v))
def test_swiglu_fwd_bwd_match_float64_autograd(rows, inter):
    """act = silu(gate) up and its float64 autograd, gate / up picked by explicit index tensors.  Catches: gate and up swapped or the
    32-column interleave computed as c // 64 or c % 64; ``1 - sig`` written as ``sig`` or a dropped ``1 +`` in dg (the block around
    g = -1.2785 and +-20 separates them); a grid-stride loop that stops after one pass (400 x 11008)."""
    ops = _ops()
    gu, dact = _swiglu_inputs(rows, inter)
    r_act, r_dgu = _swiglu_eval(gu, dact, torch.float64)
    t_act, t_dgu = _swiglu_eval(gu, dact, torch.float32)
    b_act, u_act, b_dgu, u_dgu = _swiglu_bounds(gu, dact)
    name = f"swiglu[{rows}x{inter}]"
    gug, dactg = _to(gu), _to(dact)
    a_before, a_mask = _out_slab(rows * inter, torch.bfloat16)
    d_before, d_mask = _out_slab(2 * rows * inter, torch.bfloat16)
    ab, db = _to(a_before), _to(d_before)
    act, dgu = ab[3:3 + rows * inter].view(rows, inter), db[3:3 + 2 * rows * inter].view(rows, 2 * inter)
    ops.swiglu_fwd(gug, act)
    ops.swiglu_bwd(gug, dactg, dgu)
    _sync()
    _assert_untouched(name + " act", ab, a_before, a_mask)
    _assert_untouched(name + " dgu", db, d_before, d_mask)
    _same(name + " gu", gug, gu)
    _same(name + " dact", dactg, dact)
    floor, r = _tol("swiglu fwd", t_act, r_act, b_act, under=u_act)
    print(f"[ratio] {name} act: torch fp32 {r:.3g}")
    _check(name + " act", act.float(), r_act, _bf16_ulp(r_act) + floor)
    floor, r = _tol("swiglu bwd", t_dgu, r_dgu, b_dgu, under=u_dgu)
    print(f"[ratio] {name} dgu: torch fp32 {r:.3g}")
    _check(name + " dgu", dgu.float(), r_dgu, _bf16_ulp(r_dgu) + floor)


def test_swiglu_rejects_inter_not_a_multiple_of_32():
    """inter % 32 != 0 must be refused before anything is launched (the index arithmetic assumes whole 64-column groups)"""
    ops = _ops()
    gu, dact = _to(torch.ones(2, 96)), _to(torch.ones(2, 48))
    a_before, d_before = _bf_sentinel((2, 48)), _bf_sentinel((2, 96))
    act, dgu = _to(a_before), _to(d_before)
    with pytest.raises(_err_type(), match="bad arguments"):
        ops.swiglu_fwd(gu, act)
    with pytest.raises(_err_type(), match="bad arguments"):
        ops.swiglu_bwd(gu, dact, dgu)
    _sync()
    assert torch.equal(_bits(act), _bits(a_before)) and torch.equal(_bits(dgu), _bits(d_before)), "the refused call launched a kernel"


# =====================================================================================================================
# 2. attn_ds
# =====================================================================================================================
DS_CASES = [(S, b) for S in (1, 2, 63, 64, 65, 130) for b in (1, 6)] + [(1000, 1)]
DS_SCALE = _f32(1.0 / math.sqrt(128.0))


def _attn_ds_eval(P, dP, dtype):
    """dS = P o (dP - rowsum_{j<=i}(P o dP)) scale on the lower triangle; P bf16-valued, dP with its upper triangle already zeroed"""
    p, d = P.to(dtype), dP.to(dtype)
    dot = (p * d).sum(-1, keepdim=True)
    return p * (d - dot) * DS_SCALE


@pytest.mark.parametrize("pad", [False, True], ids=["ldpS", "ldp64"])
@pytest.mark.parametrize("S,batch", DS_CASES, ids=lambda v: str(v))
def test_attn_ds_matches_float64_softmax_backward(S, batch, pad):
    """Catches: the row sum taken over the whole row (the 1e30 left above the diagonal by the full-square dO . V^T product then
    swamps it) or stopping at j < i; ``scale`` dropped or applied twice; P / dS indexed with pitch S instead of ldp; a row of the
    second wave-quartet (S = 65, 130) taking the first's dot."""
    ops = _ops()
    g = _gen(S, batch, 2)
    ldp = -(-S // 64) * 64 if pad else S
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    sc = (torch.randn(batch, S, S, generator=g) * 3).double().masked_fill(~causal, float("-inf"))
    P = torch.softmax(sc, -1).bfloat16()                                     # exact zeros above the diagonal
    dP = torch.randn(batch, S, S, generator=g)
    dP_in = dP.masked_fill(~causal, 1e30)
    dP0 = dP.masked_fill(~causal, 0.0)
    ref = _attn_ds_eval(P, dP0, torch.float64)
    bound = DS_SCALE * P.double().abs() * (dP0.double().abs() + (P.double() * dP0.double()).abs().sum(-1, keepdim=True))
    atol, r = _tol("attn_ds", _attn_ds_eval(P, dP0, torch.float32), ref, bound)
    p_host = _bf_sentinel((batch, S, ldp))                                   # pad columns of P: a NaN that must never be read
    p_host[:, :, :S] = P
    before = _bf_sentinel((batch + 1, S, ldp))
    pg, dpg, out = _to(p_host), _to(dP_in), _to(before)
    ops.attn_ds(pg, dpg, batch, S, DS_SCALE, out[:batch])
    _sync()
    name = f"attn_ds[S{S} b{batch} ldp{ldp}]"
    written = torch.zeros(before.shape, dtype=torch.bool)
    written[:batch] = True
    _assert_untouched(name, out, before, written)
    _same(name + " P", pg, p_host)
    _same(name + " dP", dpg, dP_in)
    got = out[:batch].cpu()
    dead = torch.ones(S, ldp, dtype=torch.bool)
    dead[:, :S] = ~causal
    assert not bool(_bits(got)[:, dead].any()), f"{name}: entries above the diagonal / pad columns must be exact zeros"
    print(f"[ratio] {name}: torch fp32 {r:.3g}")
    live = causal.expand(batch, S, S)
    _check(name, got[:, :, :S].float()[live], ref[live], (_bf16_ulp(ref) + atol)[live.numpy()])


# =====================================================================================================================
# 3. rope_merge_bwd
# =====================================================================================================================
ROPE_CASES = [(1, 1, 1, 0), (2, 3, 5, 0), (1, 2, 100, 37), (2, 3, 130, 24), (2, 32, 1100, 8)]   # the last: 4 505 600 pairs > GRID_CAP
HD = 128


def _rope_tables(pos0, S):
    """cos / sin [rows][64] fp32: rows [pos0, pos0 + S) hold the table, every other row (below pos0 and 3 past the end) a NaN"""
    from oracle.llama_ref import rope_cos_sin
    cos, sin = rope_cos_sin(torch.arange(pos0 + S), HD, 10000.0)
    tc, ts = _nan_buf(pos0 + S + 3, HD // 2), _nan_buf(pos0 + S + 3, HD // 2)
    tc[pos0:pos0 + S], ts[pos0:pos0 + S] = cos[pos0:, : HD // 2], sin[pos0:, : HD // 2]
    return tc, ts


def _rope_bwd_eval(d, cos, sin, dtype):
    """autograd through the forward rotate_half RoPE y = x cos + rotate_half(x) sin; d [B][nh][S][128], cos / sin [S][128]"""
    from oracle.llama_ref import _rotate_half
    x = torch.zeros(d.shape, dtype=dtype, requires_grad=True)
    (x * cos.to(dtype) + _rotate_half(x) * sin.to(dtype)).backward(d.to(dtype))
    return x.grad


def _merge(t, B, nh, S):
    return t.permute(0, 2, 1, 3).reshape(B * S, nh * HD)


@pytest.mark.parametrize("B,nh,S,pos0", ROPE_CASES, ids=lambda v: str(v))
def test_rope_merge_bwd_matches_float64_autograd_of_rope(B, nh, S, pos0):
    """Catches: a swapped sign (dx1 = dy1 c - dy2 s), the table read at row s instead of pos0 + s (those rows are NaN here), q / k /
    v thirds or heads placed at the wrong columns, dv rounded differently from RNE, a one-pass grid-stride loop (2 x 32 x 1100)."""
    ops = _ops()
    g = _gen(B, nh, S, pos0, 3)
    dq, dk, dv = (torch.randn(B, nh, S, HD, generator=g) for _ in range(3))
    tc, ts = _rope_tables(pos0, S)
    cos, sin = torch.cat((tc[pos0:pos0 + S],) * 2, -1), torch.cat((ts[pos0:pos0 + S],) * 2, -1)      # [S][128], as the forward uses them
    H = nh * HD
    name = f"rope_merge_bwd[{B}x{nh}x{S} pos0={pos0}]"
    before = _bf_sentinel((B * S + 2, 3 * H))
    out = _to(before)
    ins = [dq, dk, dv, tc, ts]
    dev = [_to(t) for t in ins]
    ops.rope_merge_bwd(dev[0], dev[1], dev[2], dev[3], dev[4], B, S, nh, HD, pos0, out[:B * S])
    _sync()
    _assert_untouched(name, out, before, _mask(before.shape, B * S, 0, 3 * H))
    for nm, a, b in zip(("dq", "dk", "dv", "cos", "sin"), dev, ins):
        _same(f"{name} {nm}", a, b)
    got = out[:B * S].cpu()
    assert torch.equal(_bits(got[:, 2 * H:]), _bits(_merge(dv, B, nh, S).bfloat16())), f"{name}: the dv third is not the RNE rounding of dv in place"
    for nm, d, c0 in (("dq", dq, 0), ("dk", dk, H)):
        ref = _merge(_rope_bwd_eval(d, cos, sin, torch.float64), B, nh, S)
        t32 = _merge(_rope_bwd_eval(d, cos, sin, torch.float32), B, nh, S)
        d64 = d.double()
        partner = torch.cat((d64[..., HD // 2:], d64[..., : HD // 2]), -1)
        bound = _merge(d64.abs() * cos.double().abs() + partner.abs() * sin.double().abs(), B, nh, S)
        floor, r = _tol(f"rope bwd {nm}", t32, ref, bound)
        print(f"[ratio] {name} {nm}: torch fp32 {r:.3g}")
        _check(f"{name} {nm}", got[:, c0:c0 + H].float(), ref, _bf16_ulp(ref) + floor)


# =====================================================================================================================
# 4. cross_entropy_shifted / cross_entropy_bwd
# =====================================================================================================================
def _ce_forward(logits, ldl, B, S, V, labels, ignore_index, row_loss, loss_out):
    from llark_amd import _lib, ops
    ops.check(_lib.lib().llark_cross_entropy_shifted(logits.data_ptr(), ldl, B, S, V, labels.data_ptr(), ignore_index, row_loss.data_ptr(),
                                                     loss_out.data_ptr(), torch.cuda.current_stream().cuda_stream), "cross_entropy_shifted")


def _ce_backward(logits, ldl, B, S, V, labels, row_loss, loss_out, loss_scale, dlogits, ldd):
    from llark_amd import _lib, ops
    ops.check(_lib.lib().llark_cross_entropy_bwd(logits.data_ptr(), ldl, B, S, V, labels.data_ptr(), row_loss.data_ptr(), loss_out.data_ptr(),
                                                 float(loss_scale), dlogits.data_ptr(), ldd, torch.cuda.current_stream().cuda_stream),
              "cross_entropy_bwd")


def _ce_case(V, ldl, B, S, ignore_index, oob=False, all_ignored=False):
    """logits [B*S + 1][ldl] (NaN outside [B*S][V]), labels [B][S], the target of every row and which rows count"""
    g = _gen(V, ldl, B, S, 4)
    rows = B * S
    logits = _nan_buf(rows + 1, ldl)
    logits[:rows, :V] = torch.randn(rows, V, generator=g) * 4
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[0, : min(3, S - 1)] = ignore_index                 # a prefix of ignore_index (the prompt)
    if S > 3:
        labels[1:, 1:3] = ignore_index                        # labels[b][0], b >= 1, stays a valid class: a kernel that walks the flat
    if oob:                                                   # label array past the end of a sequence would count row S - 1 with it
        labels[0, S - 1] = V + 17                             # in [vocab, ldl): not counted, and every address stays inside the row
    if all_ignored:
        labels[:] = ignore_index
    tgt = torch.full((B, S), ignore_index, dtype=torch.int64)
    tgt[:, :-1] = labels[:, 1:]
    tgt = tgt.flatten()
    counted = (tgt != ignore_index) & (tgt >= 0) & (tgt < V)
    counted.view(B, S)[:, -1] = False
    cr = counted.nonzero().flatten().tolist()
    others = lambda r: [c for c in range(min(V, 64)) if c != int(tgt[r])][:3]
    if len(cr) > 0:
        logits[cr[0], :V] += 1e4                              # exp overflows without the max
    if len(cr) > 1:
        logits[cr[1], :V] -= 1e4                              # everything underflows without it
        if V > 1:
            logits[cr[1], others(cr[1])] = float("-inf")      # several -inf entries off the target
    if len(cr) > 2 and V > 1:                                 # the target is the arg-max by 30: loss ~ 1e-13, the absolute floor matters
        r = cr[2]
        rest = torch.cat((logits[r, : int(tgt[r])], logits[r, int(tgt[r]) + 1:V]))
        logits[r, int(tgt[r])] = rest.max() + 30.0
    if len(cr) > 3 and V > 1:
        logits[cr[3], others(cr[3])] = float("-inf")
    return logits, labels, tgt, counted


def _ce_eval(l, tgt, counted, loss_scale, dtype, count=None):
    """(row losses of the counted rows, their mean, d mean / d logits * loss_scale over all rows) with F.cross_entropy / softmax"""
    idx = counted.nonzero().flatten()
    count = int(idx.numel()) if count is None else count
    lc, t = l[idx].to(dtype), tgt[idx]
    row = F.cross_entropy(lc, t, reduction="none")
    onehot = F.one_hot(t, l.shape[1]).to(dtype)
    dl = torch.zeros(l.shape, dtype=dtype)
    dl[idx] = (torch.softmax(lc, -1) - onehot) * loss_scale / count
    return row, row.sum() / count, dl


def _ce_bounds(l, tgt, counted, loss_scale, count=None):
    idx = counted.nonzero().flatten()
    count = int(idx.numel()) if count is None else count
    lc, t = l[idx].double(), tgt[idx]
    mx = lc.max(-1, keepdim=True).values
    b_row = mx.abs().squeeze(1) + torch.log(torch.exp(lc - mx).sum(-1)).abs() + lc.gather(1, t[:, None]).squeeze(1).abs()
    p = torch.softmax(lc, -1)
    b = torch.where(p > 0, p * ((lc - mx).abs().clamp_max(1e300) + 2.0), torch.zeros_like(p)) + F.one_hot(t, l.shape[1]).double()
    b_dl = torch.zeros(l.shape, dtype=torch.float64)
    b_dl[idx] = b * loss_scale / count
    return b_row, b_row.mean().reshape(1), b_dl


def _ce_launch(logits, labels, B, S, V, ignore_index, loss_scale, ldd):
    """both ABI calls on sentinel buffers; returns (row_loss, loss_out, dlogits) on the host after the untouched / unchanged checks"""
    rows, ldl = B * S, logits.shape[1]
    rl_before, rl_mask = _out_slab(rows, torch.float32)
    lo_before, lo_mask = _out_slab(2, torch.float32)
    dl_before = _bf_sentinel((rows + 1, ldd))
    lg, lab, rl, lo, dl = _to(logits), _to(labels), _to(rl_before), _to(lo_before), _to(dl_before)
    _ce_forward(lg, ldl, B, S, V, lab, ignore_index, rl[3:3 + rows], lo[3:5])
    _ce_backward(lg, ldl, B, S, V, lab, rl[3:3 + rows], lo[3:5], loss_scale, dl, ldd)
    _sync()
    name = f"cross_entropy[V{V} ldl{ldl} {B}x{S}]"
    _assert_untouched(name + " row_loss", rl, rl_before, rl_mask)
    _assert_untouched(name + " loss_out", lo, lo_before, lo_mask)
    _assert_untouched(name + " dlogits", dl, dl_before, _mask(dl_before.shape, rows, 0, ldd))
    _same(name + " logits", lg, logits)
    assert torch.equal(lab.cpu(), labels), f"{name}: the labels were modified"
    return name, rl[3:3 + rows].cpu(), lo[3:5].cpu(), dl[:rows].cpu()


def _ce_run(V, ldl, B, S, ignore_index, loss_scale, ldd, oob=False):
    logits, labels, tgt, counted = _ce_case(V, ldl, B, S, ignore_index, oob)
    rows = B * S
    count = int(counted.sum())
    assert count > 0
    l = logits[:rows, :V]
    r_row, r_mean, r_dl = _ce_eval(l, tgt, counted, loss_scale, torch.float64)
    t_row, t_mean, t_dl = _ce_eval(l, tgt, counted, loss_scale, torch.float32)
    b_row, b_mean, b_dl = _ce_bounds(l, tgt, counted, loss_scale)
    name, row_loss, loss_out, dl = _ce_launch(logits, labels, B, S, V, ignore_index, loss_scale, ldd)
    assert loss_out[1].item() == float(count), f"{name}: loss_out[1] = {loss_out[1].item()}, {count} rows count"
    atol, r = _tol("ce row_loss", t_row, r_row, b_row)
    _check(name + " row_loss", row_loss[counted], r_row, atol, bound=b_row, r_torch=r)
    atol, r = _tol("ce mean", t_mean.reshape(1), r_mean.reshape(1), b_mean)
    _check(name + " mean", loss_out[:1], r_mean.reshape(1), atol, bound=b_mean, r_torch=r)
    assert not bool(_bits(dl)[:, V:].any()), f"{name}: pad columns of dlogits must be exact zeros"
    assert not bool(_bits(dl)[~counted].any()), f"{name}: rows that do not count must have an exactly zero gradient"
    floor, r = _tol("ce dlogits", t_dl, r_dl, b_dl)
    print(f"[ratio] {name} dlogits: torch fp32 {r:.3g}")
    _check(name + " dlogits", dl[:, :V].float(), r_dl, _bf16_ulp(r_dl) + floor)


@pytest.mark.parametrize("variant", ["ldd=V scale1", "ldd>V scale.25"])
@pytest.mark.parametrize("B,S", [(1, 2), (2, 9), (3, 33)], ids=lambda v: str(v))
@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 1000])
def test_cross_entropy_rows_count_mean_and_gradient(V, B, S, variant):
    """row_loss vs float64 F.cross_entropy, loss_out = {mean, count}, dlogits vs loss_scale (softmax64 - onehot) / count.  Catches:
    labels[s] read instead of labels[s + 1]; the last position counted with the next sequence's first label; the max or the sum
    folded over 3 of the 4 waves, or a column >= 256 skipped (V = 255 / 256 / 257); exp without the max (rows at +-1e4); the
    gradient divided by the number of rows instead of the count, or loss_scale dropped; pad columns left unwritten."""
    pad = variant.startswith("ldd>V")
    _ce_run(V, V, B, S, -100, 0.25 if pad else 1.0, V + 5 if pad else V)


@pytest.mark.parametrize("loss_scale", [1.0, 0.25])
def test_cross_entropy_padded_vocab_and_out_of_range_target(loss_scale):
    """the real padded row: vocab 32004 in a pitch of 32064 whose pad columns hold NaN (never read: they would poison max and sum),
    and a target in [vocab, ldl), which is treated like ignore_index: not counted, zero gradient row"""
    _ce_run(32004, 32064, 1, 5, -100, loss_scale, 32064, oob=True)


def test_cross_entropy_custom_ignore_index():
    """ignore_index = 7: rows whose target is class 7 do not count (and -100 has no special meaning); catches a hard-coded -100"""
    V, B, S = 12, 3, 33
    _, labels, _, counted = _ce_case(V, V, B, S, 7)
    assert int((labels[:, 3:] == 7).sum()) > 0, "no natural occurrence of class 7: choose another seed"
    _ce_run(V, V, B, S, 7, 1.0, V + 5)


def test_cross_entropy_all_rows_ignored():
    """no row counts: loss NaN, count 0, and the backward writes zeros everywhere (it must skip every row, not divide by the count)"""
    V, B, S = 257, 2, 9
    logits, labels, tgt, counted = _ce_case(V, V, B, S, -100, all_ignored=True)
    assert not bool(counted.any())
    name, row_loss, loss_out, dl = _ce_launch(logits, labels, B, S, V, -100, 1.0, V + 5)
    assert math.isnan(loss_out[0].item()) and loss_out[1].item() == 0.0, f"{name}: loss_out = {loss_out.tolist()}"
    assert not bool(_bits(dl).any()), f"{name}: dlogits must be all zeros"


def test_cross_entropy_nan_row_counts():
    """a counted row that holds a NaN: the mean is NaN and the count unchanged, as torch reports it; every other row keeps its loss
    and its gradient (divided by the same count); the NaN row's own gradient is NaN, its pad columns zero"""
    V, B, S, ldd = 300, 2, 9, 305
    logits, labels, tgt, counted = _ce_case(V, V, B, S, -100)
    cr = counted.nonzero().flatten().tolist()
    bad = cr[-1]
    logits[bad, (int(tgt[bad]) + 1) % V] = float("nan")
    count = len(cr)
    assert math.isnan(F.cross_entropy(logits[: B * S, :V][counted], tgt[counted]).item())
    name, row_loss, loss_out, dl = _ce_launch(logits, labels, B, S, V, -100, 1.0, ldd)
    assert math.isnan(loss_out[0].item()) and loss_out[1].item() == float(count), f"{name}: loss_out = {loss_out.tolist()}"
    assert math.isnan(row_loss[bad].item())
    good = counted.clone()
    good[bad] = False
    l = logits[: B * S, :V]
    r_row, _, r_dl = _ce_eval(l, tgt, good, 1.0, torch.float64, count)
    t_row, _, t_dl = _ce_eval(l, tgt, good, 1.0, torch.float32, count)
    b_row, _, b_dl = _ce_bounds(l, tgt, good, 1.0, count)
    atol, r = _tol("ce row_loss", t_row, r_row, b_row)
    _check(name + " row_loss", row_loss[good], r_row, atol, bound=b_row, r_torch=r)
    assert bool(torch.isnan(dl[bad, :V].float()).all()) and not bool(_bits(dl)[:, V:].any())
    keep = torch.ones(B * S, dtype=torch.bool)
    keep[bad] = False
    assert not bool(_bits(dl)[~counted].any())
    floor, r = _tol("ce dlogits", t_dl[keep], r_dl[keep], b_dl[keep])
    _check(name + " dlogits", dl[keep][:, :V].float(), r_dl[keep], _bf16_ulp(r_dl[keep]) + floor)


# =====================================================================================================================
# 5. sumsq_f32
# =====================================================================================================================
SUMSQ_N = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1027, 1000003, 2200005]          # the last: 550 001 float4 > 2048 blocks x 256 threads


def _sumsq_buf(o, n, seed):
    buf = torch.full((o + n + 5,), float("nan"))
    buf[o:o + n] = torch.randn(n, generator=_gen(o, n, seed)) * 1.5
    return buf


def _sumsq_check(name, got, x):
    ref = x.double().pow(2).sum().reshape(1)
    atol, r = _tol("sumsq", x.pow(2).sum().reshape(1), ref, ref)
    _check(name, got, ref, atol, bound=ref, r_torch=r)


def _double_cell(value):
    """one double between two NaN doubles"""
    return torch.tensor([float("nan"), value, float("nan")], dtype=torch.float64)


@pytest.mark.parametrize("n", SUMSQ_N)
@pytest.mark.parametrize("o", [0, 1, 2, 3])
def test_sumsq_f32_on_unaligned_slices(o, n):
    """x = buf[o : o + n] of a 16-byte aligned buffer whose other elements are NaN (a slice of the flat gradient).  Catches: the
    ``head`` scalars (3, 2, 1 for o = 1, 2, 3) skipped, read twice or not clamped to n (o = 1 with n = 1, 2); the 0-3 element tail
    read from the wrong base; an out that is added to where it must be overwritten; the capped grid walking one pass only."""
    ops = _ops()
    buf = _sumsq_buf(o, n, 5)
    dev = _to(buf)
    cell = _double_cell(float("nan"))
    out = _to(cell)
    ops.sumsq_f32(dev[o:o + n], out[1:2], accumulate=False)                   # the NaN that was there is overwritten
    _sync()
    _same("sumsq x", dev, buf)
    assert torch.equal(_bits(out)[[0, 2]], _bits(cell)[[0, 2]]), "sumsq_f32 wrote next to its scalar"
    _sumsq_check(f"sumsq_f32[o{o} n{n}]", out[1:2], buf[o:o + n])


def test_sumsq_f32_accumulates_slices_into_one_scalar():
    """accumulate != 0 adds to the value that is there; two slices summed into one scalar give the sum of squares of the whole"""
    ops = _ops()
    n, cut = 5003, 1234 + 1                                                  # both slices start off a 16-byte boundary
    buf = _sumsq_buf(1, n, 6)
    dev = _to(buf)
    x = buf[1:1 + n]
    out = _to(_double_cell(3.5))
    ops.sumsq_f32(dev[1:1 + n], out[1:2], accumulate=True)
    _sync()
    ref = x.double().pow(2).sum().reshape(1) + 3.5
    atol, r = _tol("sumsq", (x.pow(2).sum() + 3.5).reshape(1), ref, ref)
    _check("sumsq_f32 accumulate", out[1:2], ref, atol, bound=ref, r_torch=r)
    out = _to(_double_cell(float("nan")))
    ops.sumsq_f32(dev[1:1 + cut], out[1:2], accumulate=False)
    ops.sumsq_f32(dev[1 + cut:1 + n], out[1:2], accumulate=True)
    _sync()
    _sumsq_check("sumsq_f32 two slices", out[1:2], x)
    fresh = ops.sumsq_f32(dev[1:1 + n])                                     # no out: a new scalar
    _sumsq_check("sumsq_f32 fresh scalar", fresh, x)


@pytest.mark.parametrize("n", [1, 6, 1027])
def test_sumsq_f32_of_zeros_is_exactly_zero(n):
    ops = _ops()
    out = _to(_double_cell(float("nan")))
    ops.sumsq_f32(_to(torch.zeros(n + 1))[1:], out[1:2], accumulate=False)
    _sync()
    assert out[1].item() == 0.0


# =====================================================================================================================
# 6. adamw, adamw_clip, adamw_twins
# =====================================================================================================================
B1, B2, ADAM_EPS = _f32(0.9), _f32(0.999), _f32(1e-8)
# (step, weight_decay, lr, grad_scale): every value of each hyperparameter, not the full product
ADAMW_HYPER = [(1, 0.0, 1e-2, 1.0), (1, 0.1, 5e-5, 0.25), (2, 0.1, 1e-2, 1.0), (2, 0.0, 5e-5, 0.25), (1000, 0.1, 1e-2, 0.25),
               (100000, 0.0, 1e-2, 1.0), (100000, 0.1, 5e-5, 1.0)]


def _adamw_torch(p, g, m, v, step, lr, wd, dtype, betas=(B1, B2), eps=ADAM_EPS):
    """one torch.optim.AdamW step number ``step`` from the given moments (loaded through load_state_dict): (p, exp_avg, exp_avg_sq)"""
    P = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.AdamW([P], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    sd = opt.state_dict()
    sd["state"] = {0: {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}}
    opt.load_state_dict(sd)
    P.grad = g.to(dtype)
    opt.step()
    st = opt.state[P]
    assert float(st["step"]) == float(step)
    return P.detach(), st["exp_avg"], st["exp_avg_sq"]


def _adamw_state(n, bf16, seed):
    g_ = _gen(n, seed, 6)
    p, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    m, v = torch.randn(n, generator=g_) * 1e-2, (torch.randn(n, generator=g_) * 1e-2) ** 2
    if n >= 48:
        g[0:16], m[0:16], v[0:16] = 0.0, 0.0, 0.0            # only the decay applies; 0 / (0 + eps) must stay finite
        g[16:32] *= 1e-8                                     # denominator dominated by eps
        m[16:32], v[16:32] = 0.0, 0.0
        g[32:48] *= 1e3
    return (p.bfloat16() if bf16 else p), g, m, v


def _clip_coef(sumsq, grad_scale, max_norm):
    return min(1.0, max_norm / (math.sqrt(sumsq) * grad_scale + 1e-6))


def _run_adamw(name, p, g, m, v, hyper, sumsq=None, max_norm=0.0, sumsq_on_device=False, twins=None):
    """launch adamw / adamw_clip / adamw_twins on slices inside sentinel buffers and compare p, m, v with float64 torch.optim.AdamW;
    returns (reference m, tolerance of m, updated device p, wfrag, wtfrag) for the callers that assert more"""
    ops = _ops()
    step, wd, lr, gs = hyper
    lr, wd = _f32(lr), _f32(wd)
    coef = 1.0 if sumsq is None else _clip_coef(sumsq, gs, max_norm)
    g_eff = g.double() * gs * coef
    r_p, r_m, r_v = _adamw_torch(p, g_eff, m, v, step, lr, wd, torch.float64)
    t_p, t_m, t_v = _adamw_torch(p, g * _f32(gs * coef), m, v, step, lr, wd, torch.float32)
    u_p, _, _ = _adamw_torch(p, g_eff, m, v, step, hyper[2], hyper[1], torch.float64, betas=(0.9, 0.999), eps=1e-8)
    mhat, vhat = r_m / (1.0 - B1 ** step), r_v / (1.0 - B2 ** step)
    b_p = p.double().abs() + lr * mhat.abs() / (vhat.sqrt() + ADAM_EPS)
    b_m = B1 * m.double().abs() + (1.0 - B1) * g_eff.abs()
    b_v = B2 * v.double() + (1.0 - B2) * g_eff ** 2
    front = 8 if twins else 3                               # adamw_twins needs 16-byte aligned pointers
    bufs = [_slab(t, front, front + 1) for t in (p, g, m, v)]
    (pb, pm), (gb, _), (mb, mm), (vb, vm) = bufs
    dev = [_to(b) for b, _ in bufs]
    n = p.numel()
    pd, gd, md, vd = (d[front:front + n] for d in dev)
    ss = None
    if sumsq is not None:
        ss = ops.sumsq_f32(gd) if sumsq_on_device else _to(torch.tensor([sumsq], dtype=torch.float64))
    wf = wtf = None
    if twins:
        rows, k, rope_rows = twins
        wf_before, wf_mask = _out_slab(n, torch.bfloat16, 8, 8)
        wf = _to(wf_before)
        wtf = _to(wf_before) if rows % 64 == 0 else None
        pd = pd.view(rows, k)
        ops.adamw_twins(pd, gd, md, vd, lr, B1, B2, ADAM_EPS, wd, step, gs, grad_sumsq=ss, max_grad_norm=max_norm,
                        wfrag=wf[8:8 + n], rope_rows=rope_rows, wtfrag=None if wtf is None else wtf[8:8 + n])
    else:
        ops.adamw(pd, gd, md, vd, lr, B1, B2, ADAM_EPS, wd, step, gs, grad_sumsq=ss, max_grad_norm=max_norm)
    _sync()
    for nm, d, b, msk in (("p", dev[0], pb, pm), ("m", dev[2], mb, mm), ("v", dev[3], vb, vm)):
        _assert_untouched(f"{name} {nm}", d, b, msk)
    _same(name + " g", dev[1], gb)
    if twins:
        for t in (wf, wtf):
            if t is not None:
                _assert_untouched(name + " twin", t, wf_before, wf_mask)
    atol_m, r = _tol("adamw m", t_m, r_m, b_m)
    _check(name + " m", md, r_m, atol_m, bound=b_m, r_torch=r)
    atol, r = _tol("adamw v", t_v, r_v, b_v)
    _check(name + " v", vd, r_v, atol, bound=b_v, r_torch=r)
    atol, r = _tol("adamw p", t_p, r_p, b_p)
    print(f"[ratio] {name} p: unrounded Python hyperparameters are {float(((u_p - r_p).abs() / (EPS24 * b_p))[b_p > 0].max()):.3g} x 2^-24 B away")
    if p.dtype == torch.bfloat16:
        print(f"[ratio] {name} p: torch fp32 {r:.3g}")
        _check(name + " p", pd.reshape(-1).float(), r_p, _bf16_ulp(r_p) + atol)
    else:
        _check(name + " p", pd, r_p, atol, bound=b_p, r_torch=r)
    return r_m, atol_m, pd, wf, wtf


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hyper", ADAMW_HYPER, ids=lambda h: "step{}-wd{}-lr{}-gs{}".format(*h))
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_adamw_matches_float64_torch_adamw(n, hyper, bf16):
    """p, exp_avg and exp_avg_sq after step number ``step`` from arbitrary moments.  Catches: a missing or coupled weight decay
    (wd = 0.1 moves p by lr wd |p|, far outside 16 x 2^-24 |p| in fp32); eps inside the square root (the |g| ~ 1e-8 block); bias
    corrections swapped, taken at step - 1 or dropped (steps 1 and 2); grad_scale applied to m only or not squared in v; the fp32
    kernel rounding p through bf16."""
    p, g, m, v = _adamw_state(n, bf16, 1)
    _run_adamw(f"adamw[{'bf16' if bf16 else 'fp32'} n{n} step{hyper[0]} wd{hyper[1]} lr{hyper[2]} gs{hyper[3]}]", p, g, m, v, hyper)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_adamw_walks_more_than_one_pass_of_its_grid(bf16):
    n = GRID_CAP + 257
    p, g, m, v = _adamw_state(n, bf16, 2)
    _run_adamw(f"adamw[{'bf16' if bf16 else 'fp32'} n{n}]", p, g, m, v, (2, 0.1, 1e-2, 0.25))


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("coef", [0.05, 0.999, 1.001, 20.0, "device"])
def test_adamw_clip_applies_the_clip_grad_norm_coefficient(coef, bf16):
    """the gradient is multiplied by grad_scale min(1, max_norm / (sqrt(sumsq) grad_scale + 1e-6)): coefficients 0.05 and 0.999
    clip, 1.001 and 20 must leave the gradient alone; "device": sumsq comes from sumsq_f32 over the gradient and clips to ~0.05.
    Catches a clip that is not applied (the unclipped float64 reference is asserted to lie outside the tolerance at 0.05), one
    applied above 1, the 1e-6 or grad_scale missing from the norm."""
    n, gs, max_norm = 4097, 0.25, 1.0
    p, g, m, v = _adamw_state(n, bf16, 3)
    hyper = (2, 0.1, 1e-2, gs)
    if coef == "device":
        sumsq = float(g.double().pow(2).sum())
        max_norm = _f32(0.05 * (math.sqrt(sumsq) * gs + 1e-6))
    else:
        sumsq = ((max_norm / coef - 1e-6) / gs) ** 2
        assert abs(max_norm / (math.sqrt(sumsq) * gs + 1e-6) - coef) < 1e-9 * coef
    name = f"adamw_clip[{'bf16' if bf16 else 'fp32'} coef {coef}]"
    r_m, atol_m, _, _, _ = _run_adamw(name, p, g, m, v, hyper, sumsq=sumsq, max_norm=max_norm, sumsq_on_device=coef == "device")
    if coef in (0.05, "device"):
        _, unclipped_m, _ = _adamw_torch(p, g.double() * gs, m, v, 2, _f32(1e-2), _f32(0.1), torch.float64)
        outside = ((unclipped_m - r_m).abs().numpy() > atol_m).mean()
        assert outside > 0.9, f"{name}: the tolerance would accept a missing clip ({outside:.2f} of the elements tell them apart)"


@pytest.mark.parametrize("rows,k,rope_rows", [(32, 128, 0), (64, 256, 0), (128, 128, 128), (256, 384, 128)], ids=lambda v: str(v))
def test_adamw_twins_matches_float64_torch_adamw_and_packs_the_result(rows, k, rope_rows):
    """p, m, v of llark_adamw_twins against the same float64 reference (not against llark_adamw), and the two twins against
    pack_weight16_frag of the updated weight (rows below rope_rows in the fused-RoPE order) and of its transpose.  Catches: a tile
    indexed with the wrong pitch (k = 256, 384: more than one column tile), the decay factor or a bias correction dropped from the
    restated arithmetic, the head permutation applied at or above rope_rows (256 rows, rope_rows 128)."""
    ops = _ops()
    n = rows * k
    p, g, m, v = _adamw_state(n, True, 4)
    p = (p.float() * 0.05).bfloat16()
    clip = rows >= 128
    sumsq = ((1.0 / 0.05 - 1e-6) / 0.25) ** 2 if clip else None
    _, _, pd, wf, wtf = _run_adamw(f"adamw_twins[{rows}x{k} rope{rope_rows}]", p, g, m, v, (3, 0.1, 1e-2, 0.25), sumsq=sumsq,
                                   max_norm=1.0 if clip else 0.0, twins=(rows, k, rope_rows))
    assert not torch.equal(pd.cpu().view(-1), p)
    inside = torch.cat((torch.arange(0, 32), torch.arange(64, 96), torch.arange(32, 64), torch.arange(96, 128)))
    order = torch.arange(rows)
    for h in range(rope_rows // 128):
        order[128 * h:128 * h + 128] = 128 * h + inside
    assert torch.equal(_bits(wf[8:8 + n]), _bits(ops.pack_weight16_frag(pd.index_select(0, _to(order)), rows))), "wfrag is not the packed updated weight"
    if wtf is not None:
        assert torch.equal(_bits(wtf[8:8 + n]), _bits(ops.pack_weight16_frag(ops.transposed16(pd), k))), "wtfrag is not the packed transpose"


# =====================================================================================================================
# 7. rmsnorm_bwd / rmsnorm_bwd_out16
# =====================================================================================================================
RMS_EPS = _f32(1e-5)
RMS_WIDTHS = [4, 256, 260, 1024, 1028, 2048, 2052, 4092, 4096, 4100, 8192]   # NV = 1 | 4 | 16 | the 4-waves-per-row kernel | 16 | 32
RMS_SHAPES = [(r, w) for w in RMS_WIDTHS for r in (1, 2, 3, 5)] + \
    [(2049, 256), (2049, 1028),                                              # a second pass of the 512 x 4-row grid
     (1025, 2052), (1100, 2052), (1025, 4096), (1100, 4096)]                 # a second iteration of rmsnorm_bwd2_kernel (512 x 2 rows), dead slot in the last


def _rms_inputs(rows, width):
    g = _gen(rows, width, 7)
    x = torch.randn(rows, width, generator=g) * 1.3
    scale = torch.tensor([1.0, 1e-3, 1e3])[torch.arange(rows) % 3]           # 1e-3: mean x^2 ~ 1e-6 < eps, eps decides rstd
    x = x * scale[:, None]
    dy = torch.randn(rows, width, generator=g)
    w = torch.randn(width, generator=g)
    if rows >= 5:
        x[3] = 0.0                                                          # rstd = eps ** -0.5
        dy[4] = 0.0
    if rows >= 1025:
        x[1024:1028] = 0.0                                                  # zero rows in the second pass as well
        dy[rows - 1] = 0.0
    return x, w, dy


def _rms_eval(x, w, dy, dx0, dw0, dtype):
    xx, ww = x.to(dtype).clone().requires_grad_(True), w.to(dtype).clone().requires_grad_(True)
    (ww * xx * torch.rsqrt(xx.pow(2).mean(-1, keepdim=True) + RMS_EPS)).backward(dy.to(dtype))
    return xx.grad + dx0.to(dtype), ww.grad + dw0.to(dtype)


def _rms_bounds(x, w, dy, dx0, dw0):
    x64, dy64 = x.double(), dy.double()
    rstd = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + RMS_EPS)
    xh, g = x64 * rstd, dy64 * w.double()
    b_dx = rstd * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)) + dx0.double().abs()
    b_dw = (dy64 * xh).abs().sum(0) + dw0.double().abs()
    return b_dx, b_dw


@pytest.mark.parametrize("variant", ["plain", "acc", "out16", "out16_pad_acc"])
@pytest.mark.parametrize("rows,width", RMS_SHAPES, ids=lambda v: str(v))
def test_rmsnorm_bwd_matches_float64_autograd(rows, width, variant):
    """dx (=, +=) and dw (+=) vs float64 autograd of w x rsqrt(mean(x^2) + eps); dx16 = the RNE bf16 of the fp32 dx of the same call.
    Catches: eps outside the square root or the mean taken over the padded lane count (rows scaled 1e-3, all-zero rows); a stale
    ``sred`` slot or a dead row slot that stores on the second iteration of the wide kernel (1025 / 1100 rows); dw partials lost
    between passes (2049 rows); accumulate ignored or applied to dw's partial; dx16 written with pitch width, or before the
    accumulation; the NV = 16 one-wave instantiation (1028, 2048) dropping its upper columns."""
    ops = _ops()
    accumulate, out16 = variant.endswith("acc"), variant.startswith("out16")
    x, w, dy = _rms_inputs(rows, width)
    g = _gen(rows, width, 8)
    dx0 = torch.randn(rows, width, generator=g) if accumulate else torch.zeros(rows, width)
    dw0 = torch.randn(width, generator=g)
    r_dx, r_dw = _rms_eval(x, w, dy, dx0, dw0, torch.float64)
    t_dx, t_dw = _rms_eval(x, w, dy, dx0, dw0, torch.float32)
    b_dx, b_dw = _rms_bounds(x, w, dy, dx0, dw0)
    name = f"rmsnorm_bwd[{rows}x{width} {variant}]"
    dx_before = _nan_buf(rows + 2, width)
    if accumulate:
        dx_before[:rows] = dx0
    dw_before, dw_mask = _slab(dw0)
    ld16 = width + 12 if variant == "out16_pad_acc" else width
    d16_before = _bf_sentinel((rows + 1, ld16))
    xg, wg, dyg, dxg, dwg, d16g = (_to(t) for t in (x, w, dy, dx_before, dw_before, d16_before))
    ops.rmsnorm_bwd(xg, wg, dyg, RMS_EPS, dxg[:rows], accumulate, dwg[3:3 + width], d16g[:rows] if out16 else None)
    _sync()
    _assert_untouched(name + " dx", dxg, dx_before, _mask(dx_before.shape, rows, 0, width))
    _assert_untouched(name + " dw", dwg, dw_before, dw_mask)
    _assert_untouched(name + " dx16", d16g, d16_before, _mask(d16_before.shape, rows if out16 else 0, 0, width))
    for nm, a, b in (("x", xg, x), ("w", wg, w), ("dy", dyg, dy)):
        _same(f"{name} {nm}", a, b)
    atol, r = _tol("rmsnorm_bwd dx", t_dx, r_dx, b_dx)
    _check(name + " dx", dxg[:rows], r_dx, atol, bound=b_dx, r_torch=r)
    atol, r = _tol("rmsnorm_bwd dw", t_dw, r_dw, b_dw)
    _check(name + " dw", dwg[3:3 + width], r_dw, atol, bound=b_dw, r_torch=r)
    if out16:
        assert torch.equal(_bits(d16g[:rows, :width]), _bits(dxg[:rows].cpu().bfloat16())), f"{name}: dx16 is not the RNE bf16 of the dx this call wrote"


@pytest.mark.parametrize("width,message", [(6, "multiple of 4"), (8196, "too large")])
def test_rmsnorm_bwd_rejects_unsupported_widths(width, message):
    ops = _ops()
    z = _to(torch.zeros(4, width))
    dx_before, dw_before, d16_before = _nan_buf(4, width), torch.full((width,), 0.5), _bf_sentinel((4, -(-width // 4) * 4))
    dx, dw, d16 = _to(dx_before), _to(dw_before), _to(d16_before)
    for o16 in (None, d16):
        with pytest.raises(_err_type(), match=message):
            ops.rmsnorm_bwd(z, _to(torch.ones(width)), z, RMS_EPS, dx, False, dw, o16)
    _sync()
    assert torch.equal(_bits(dx), _bits(dx_before)) and torch.equal(_bits(dw), _bits(dw_before)) and torch.equal(_bits(d16), _bits(d16_before)), \
        "the refused call launched a kernel"
