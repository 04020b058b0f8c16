"""The variable-length attention entry points with ALiBi -- llark_attn_prefill_bf16_lse_varlen_alibi and
llark_attn_backward_bf16_varlen_alibi (csrc/llama.hip, csrc/attn_bwd.hip): the ``ALIBI = true, VARLEN = true`` instantiations of the
kernels behind llark_attn_prefill_bf16_lse / llark_attn_backward_bf16.

As in test_attn_varlen_kernels_gpu.py (whose slabs, sentinels and tables are used here) the main check is BIT EQUALITY: for every
sequence of a table, ``out``, ``lse``, ``dsum``, ``dq``, ``dk``, ``dv`` equal what the uniform entry points give with the same slopes at
``batch = 1, s = len_b`` on copies of that sequence's rows.  The slopes are those of the MPT engine (``alibi_slopes(nh, 8)``), distinct
per head: a slope taken from the wrong head (``bhid`` instead of ``bhid % nh``), or a bias formed with ``max_len`` or ``s_total`` in
place of ``len_b``, moves ``lse`` by slope * (difference) -- at least 2^-8 * 1 here, far above one fp32 ulp -- and the backward's P with
it.  Rows of no sequence and the slab borders are bit-unchanged, inputs are bit-unchanged, a second launch repeats the first, a larger
``max_len`` gives the same bits.

Float64: the forward on ``tiles`` under llama_kernel_ref.check_out / check_lse and dq / dk / dv / dsum on ``gaps`` under
attn_bwd_ref.check -- the bounds the uniform kernels are held to, no tolerance of this file's own.  The references are the contract
functions of those two modules with ``slopes``; that they state ``q k^T / sqrt(128) + slope_h (key - (len_b - 1))``, causal, is asserted
here against the formula written out.

Declines: a null slope pointer and every scalar rule return LLARK_ERR_INVALID before any launch; the ops wrappers name the table rule
that a host list breaks.
"""
import math
import re

import pytest
import torch

import attn_bwd_ref as BR
import llama_kernel_ref as R
from kernel_util import bits as _bits
from test_attn_varlen_kernels_gpu import BF, DEV, ERR_INVALID, F32, HD, SPARE, TABLES, _lib, _operands, _ops, _row_mask, _Slab, _slice_of, _stream

pytestmark = pytest.mark.gpu

OUTPUTS = ("out", "lse", "dsum", "dq", "dk", "dv")


def _slopes(nh):
    from llark_amd.m2t.mpt_engine import alibi_slopes
    s = alibi_slopes(nh, 8)
    assert len(set(s.tolist())) == nh                                  # distinct per head
    return s


def _launch(D, table, max_len):
    """forward then backward (on the forward's own o / lse) through the ops wrappers; returns the slabs"""
    ops = _ops()
    nh, s_total = D["nh"], D["s_total"]
    sp = SPARE * nh * HD
    S = {k: _Slab(D[k].shape, BF, sp, D[k]) for k in ("q", "kc", "vt", "v_rm", "do_hm")}
    S["slopes"] = _Slab((nh,), F32, 8, _slopes(nh))
    S["out"] = _Slab((s_total, nh * HD), BF, sp)
    S["lse"] = _Slab((nh, s_total), F32, SPARE)
    seqs = torch.tensor(table, dtype=torch.int32).to(DEV)
    ops.attn_prefill_lse_varlen(S["q"].view, S["kc"].view, S["vt"].view, seqs, table, max_len, s_total, nh, HD, S["out"].view, S["lse"].view,
                                alibi_slopes=S["slopes"].view)
    torch.cuda.synchronize()
    S["o_in"], S["lse_in"] = _Slab(S["out"].shape, BF, sp, S["out"].view.cpu()), _Slab(S["lse"].shape, F32, SPARE, S["lse"].view.cpu())
    S["dsum"] = _Slab((nh, s_total), F32, SPARE)
    for k in ("dq", "dk", "dv"):
        S[k] = _Slab((nh, s_total, HD), F32, sp)
    ops.attn_backward_varlen(S["q"].view, S["kc"].view, S["v_rm"].view, S["do_hm"].view, S["o_in"].view, S["lse_in"].view, S["dsum"].view, seqs, table,
                             max_len, s_total, nh, HD, S["dq"].view, S["dk"].view, S["dv"].view, alibi_slopes=S["slopes"].view)
    torch.cuda.synchronize()
    return S


def _results(D, S, table):
    """host copies of every output after the untouched-outside-the-sequences check; inputs bit-unchanged"""
    nh, s_total = D["nh"], D["s_total"]
    rows = _row_mask(table, s_total)
    written = {"out": rows[:, None].expand(s_total, nh * HD), "lse": rows[None, :].expand(nh, s_total),
               "dq": rows[None, :, None].expand(nh, s_total, HD)}
    written.update(dsum=written["lse"], dk=written["dq"], dv=written["dq"])
    got = {k: S[k].result(k, written[k]) for k in OUTPUTS}
    for k in ("q", "kc", "vt", "v_rm", "do_hm", "o_in", "lse_in", "slopes"):
        S[k].unchanged(k)
    return got


def _uniform(D, off, ln, o_b, lse_b):
    """llark_attn_prefill_bf16_lse / llark_attn_backward_bf16 with the same slopes at batch = 1, s = ln on copies of rows off .. off + ln - 1"""
    ops = _ops()
    nh = D["nh"]
    smax_b = R.round_up(ln, 8) + 8
    sl = slice(off, off + ln)
    slopes = _slopes(nh).to(DEV)
    q = D["q"][:, sl].contiguous().to(DEV)
    kc = R.k_cache(D["kc"][:, sl].contiguous(), 1, nh, smax_b).to(DEV)
    vt = R.vt_cache(D["v_rm"][:, sl].contiguous(), 1, nh, smax_b).to(DEV)
    v_rm = D["v_rm"][:, sl].contiguous().to(DEV)
    do_hm = D["do_hm"][:, sl].contiguous().to(DEV)
    out = torch.empty(ln, nh * HD, dtype=BF, device=DEV)
    lse = torch.empty(nh, ln, dtype=F32, device=DEV)
    ops.attn_prefill_lse(q.view(1, nh, ln, HD), kc, vt, 1, ln, nh, HD, out, lse, alibi_slopes=slopes)
    o_in, lse_in = o_b.contiguous().to(DEV), lse_b.contiguous().to(DEV)
    dsum = torch.empty_like(lse)
    dq, dk, dv = (torch.empty(nh, ln, HD, dtype=F32, device=DEV) for _ in range(3))
    ops.attn_backward(q, kc, v_rm, do_hm, o_in, lse_in, dsum, 1, ln, nh, HD, dq, dk, dv, alibi_slopes=slopes)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(out=out, lse=lse, dsum=dsum, dq=dq, dk=dk, dv=dv).items()}


@pytest.mark.parametrize("name", list(TABLES))
def test_varlen_alibi_bit_equal_to_uniform_alibi_per_sequence(name):
    D = _operands(name)
    table = D["table"]
    max_len = max(n for _, n in table)
    got = _results(D, _launch(D, table, max_len), table)
    for k in OUTPUTS:
        sel = _slice_of(k, got[k], 0, D["s_total"])
        inside = sel[D["rows"]] if k == "out" else sel[:, D["rows"]]
        assert not bool(torch.isnan(inside.float()).any()), f"{k}: a sentinel inside a sequence"
    for b, (off, ln) in enumerate(table):
        ref = _uniform(D, off, ln, _slice_of("out", got["out"], off, ln), _slice_of("lse", got["lse"], off, ln))
        for k in OUTPUTS:
            a, r = _bits(_slice_of(k, got[k], off, ln).contiguous()), _bits(ref[k])
            assert torch.equal(a, r), f"{name}: {k} of sequence {b} (off {off}, len {ln}): {int((a != r).sum())} of {a.numel()} elements differ from the uniform ALiBi call"
    again = _results(D, _launch(D, table, max_len), table)
    for k in OUTPUTS:
        assert torch.equal(_bits(again[k]), _bits(got[k])), f"{k}: the second launch differs from the first"
    wide = _results(D, _launch(D, table, min(D["s_total"], max_len + 70)), table)
    for k in OUTPUTS:
        assert torch.equal(_bits(wide[k]), _bits(got[k])), f"{k}: differs with a larger max_len"


def _formula(q, k, v, slopes):
    """out, lse of one sequence in float64, written out: scores q k^T / sqrt(128) + slope_h (key - (len - 1)), causal"""
    n = q.shape[1]
    s = torch.matmul(q.double(), k.double().transpose(1, 2)) / math.sqrt(128.0)
    s = s + slopes.double()[:, None, None] * (torch.arange(n) - (n - 1)).double()[None, None, :]
    s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(n)[:, None], float("-inf"))
    return torch.matmul(torch.softmax(s, -1), v.double()), torch.logsumexp(s, -1)


def test_varlen_alibi_forward_against_float64():
    D = _operands("tiles")
    table, nh = D["table"], D["nh"]
    slopes = _slopes(nh)
    got = _results(D, _launch(D, table, max(n for _, n in table)), table)
    for b, (off, ln) in enumerate(table):
        sl = slice(off, off + ln)
        q, k, v = D["q"][:, sl], D["kc"][:, sl], D["v_rm"][:, sl]
        ref = R.reference(q.double(), k.double(), v.double(), 0, slopes)
        out64, lse64 = _formula(q, k, v, slopes)
        assert torch.allclose(ref.out, out64, rtol=0, atol=1e-12) and torch.allclose(ref.lse, lse64, rtol=0, atol=1e-12)
        R.check_out(f"varlen alibi out, sequence {b}", "lse", R.from_rows(got["out"][sl].double(), 1, nh), ref)
        R.check_lse(f"varlen alibi lse, sequence {b}", got["lse"][:, sl].double(), ref)


def test_varlen_alibi_backward_against_float64():
    D = _operands("gaps")
    table, nh = D["table"], D["nh"]
    slopes = _slopes(nh)
    got = _results(D, _launch(D, table, max(n for _, n in table)), table)
    for b, (off, ln) in enumerate(table):
        sl = slice(off, off + ln)
        q, k, v, dO = D["q"][:, sl], D["kc"][:, sl], D["v_rm"][:, sl], D["do_hm"][:, sl]
        o, lse = R.from_rows(got["out"][sl], 1, nh), got["lse"][:, sl]
        ref = BR.reference(q, k, v, dO, o, lse, slopes)
        # the contract function with slopes is the formula written out: P = exp(scores + bias - lse), bias slope_h (key - (len - 1))
        s = torch.matmul(q.double(), k.double().transpose(1, 2)) / math.sqrt(128.0)
        s = s + slopes.double()[:, None, None] * (torch.arange(ln) - (ln - 1)).double()[None, None, :]
        p = torch.exp(s - lse.double()[..., None]).masked_fill(torch.arange(ln)[None, :] > torch.arange(ln)[:, None], 0.0)
        assert torch.allclose(ref.dv, torch.matmul(p.transpose(1, 2), dO.double()), rtol=0, atol=1e-12)
        BR.check(f"varlen alibi, sequence {b}", {n: got[n][:, sl] for n in ("dq", "dk", "dv", "dsum")}, ref)


def test_varlen_alibi_declines_before_any_launch():
    L = _lib()
    x = torch.zeros(64, device=DEV)                                     # any valid device pointer: nothing is launched
    p, st = x.data_ptr(), _stream()

    def fwd(q=p, seqs=p, nseq=1, max_len=8, s_total=8, nh=2, hd=HD, smax=8, slopes=p):
        return L.llark_attn_prefill_bf16_lse_varlen_alibi(q, p, p, seqs, nseq, max_len, s_total, nh, hd, smax, p, p, slopes, st)

    def bwd(q=p, seqs=p, nseq=1, max_len=8, s_total=8, nh=2, hd=HD, smax=8, slopes=p):
        return L.llark_attn_backward_bf16_varlen_alibi(q, p, p, p, p, p, p, seqs, nseq, max_len, s_total, nh, hd, smax, p, p, p, slopes, st)

    for name, f in (("attn_prefill_lse_varlen_alibi", fwd), ("attn_backward_varlen_alibi", bwd)):
        for what, kw in (("null pointer", dict(slopes=None)), ("head_dim", dict(hd=64)), ("bad shape", dict(smax=12, s_total=8)),
                         ("bad shape", dict(s_total=16, smax=8)), ("bad shape", dict(max_len=16)), ("bad shape", dict(nseq=0)),
                         ("bad shape", dict(nh=0)), ("bad shape", dict(max_len=0)), ("null pointer", dict(q=None)), ("null pointer", dict(seqs=None))):
            assert f(**kw) == ERR_INVALID, (name, kw)
            msg = L.llark_last_error().decode()
            assert msg.startswith(name + ":") and what in msg, (name, kw, msg)
    torch.cuda.synchronize()
    assert bool((x == 0).all())


def test_varlen_alibi_wrappers_name_the_table_rule():
    ops = _ops()
    D = _operands("gaps")
    nh, s_total = D["nh"], D["s_total"]
    slopes = _slopes(nh).to(DEV)
    for table, max_len, says in (([(4, 8)], 8, "off % 8"), ([(0, 16), (8, 16)], 16, "disjoint"), ([(s_total - 8, 16)], 16, "off + len <= s_total"),
                                 ([(0, 16), (16, 24)], 16, "max_len >= max"), ([(0, 0)], 8, "len >= 1"), ([], 8, "empty")):
        seqs = torch.zeros((max(len(table), 1), 2), dtype=torch.int32, device=DEV)
        t = torch.zeros(8, device=DEV)
        with pytest.raises(ValueError, match=re.escape(says)):
            ops.attn_prefill_lse_varlen(t, t, t, seqs, table, max_len, s_total, nh, HD, t, t, alibi_slopes=slopes)
        with pytest.raises(ValueError, match=re.escape(says)):
            ops.attn_backward_varlen(t, t, t, t, t, t, t, seqs, table, max_len, s_total, nh, HD, t, t, t, alibi_slopes=slopes)
