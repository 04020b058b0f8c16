"""The variable-length (packed) attention entry points -- llark_attn_prefill_bf16_lse_varlen, llark_attn_backward_bf16_varlen,
llark_attn_backward_bf16_fused_varlen (csrc/llama.hip, csrc/attn_bwd.hip) -- against the uniform entry points they are a prologue of.

The uniform kernels are held to float64 references element by element (test_llama_kernels_gpu.py, test_attn_bwd_kernels_gpu.py) and the
variable-length forms leave their tile arithmetic alone, so the check here is BIT EQUALITY: for every sequence of a table, ``out``, ``lse``,
``dsum``, fp32 ``dq`` / ``dk`` / ``dv`` and the fused ``dqkv`` equal what the uniform entry point gives with ``batch = 1, s = len_b`` on copies
of that sequence's rows.  Every output lies in a NaN / sentinel slab: rows of no sequence and the slab's borders must be bit-unchanged.
Rows of no sequence hold a NaN sentinel in q, v_rm, dO, o and lse and the largest finite bf16 in the K and V^T caches, so a read outside a
sequence shows; inputs must be bit-unchanged; a second launch must repeat the first bit for bit.  One float64 check of the forward on
the first table uses the bounds of test_llama_kernels_gpu.py (llama_kernel_ref.check_out / check_lse), not a tolerance of its own.

Tables: (0, 64), (64, 8), (72, 136), (208, 72) -- exactly one tile, less than a tile, three tiles with a ragged tail whose middle tile
stands alone, neighbours directly behind a ragged tail; (8, 1), (16, 130), (152, 63) -- a gap in front and between sequences; nine
sequences of 72 rows at nh = 8 -- the XCD numbering branch (nseq * nh % 8 == 0) with nseq * nh no power of two.

Declines: the scalar rules return LLARK_ERR_INVALID before any launch; the ops wrappers name the table rule that a host list breaks; a
table entry that breaks a rule, given straight to the C entry points, leaves every output bit-unchanged for that entry while its
neighbours are computed (every tensor is allocated with spare rows behind it, so the entry points inside the allocations either way).
"""
import functools
import re

import pytest
import torch

import llama_kernel_ref as R
from kernel_util import BF_SENTINEL, assert_untouched as _assert_untouched, bf_sentinel as _bf_sentinel, bits as _bits, gen as _gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = R.HD
BF, F32 = torch.bfloat16, torch.float32
PAD = 8                    # elements in front of a tensor inside its slab: keeps the 16-byte alignment
SPARE = 16                 # rows allocated behind every tensor (sentinel): a table entry that runs past s_total stays inside the allocation
MAX_POS = 256
ERR_INVALID = -1

TABLES = {
    "tiles": (2, [(0, 64), (64, 8), (72, 136), (208, 72)]),
    "gaps": (2, [(8, 1), (16, 130), (152, 63)]),
    "xcd": (8, [(72 * i, 72) for i in range(9)]),
}


def _ops():
    from llark_amd import ops
    return ops


def _lib():
    from llark_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Slab:
    """a tensor of ``shape`` inside a sentinel slab (NaN for fp32, a NaN bf16 for bf16) with ``spare`` more sentinel elements behind it"""

    def __init__(self, shape, dtype, spare, fill=None):
        n = 1
        for d in shape:
            n *= d
        size = PAD + n + spare + PAD
        self.host = _bf_sentinel((size,)) if dtype == BF else torch.full((size,), float("nan"), dtype=dtype)
        if fill is not None:
            self.host[PAD:PAD + n] = fill.reshape(-1)
        self.dev = self.host.to(DEV)
        self.n, self.shape = n, tuple(shape)
        self.view = self.dev[PAD:PAD + n].view(*shape)

    def result(self, name, written):
        """the tensor on the host after asserting that everything outside ``written`` (a boolean of the tensor's shape) is bit-unchanged"""
        m = torch.zeros(self.host.numel(), dtype=torch.bool)
        m[PAD:PAD + self.n] = written.reshape(-1)
        _assert_untouched(name, self.dev, self.host, m)
        return self.dev.cpu()[PAD:PAD + self.n].view(*self.shape)

    def unchanged(self, name):
        assert torch.equal(_bits(self.dev), _bits(self.host)), f"{name}: an input was modified"


def _geometry(table):
    s_total = R.round_up(max(o + n for o, n in table), 8) + 8
    return s_total, s_total + 8


def _row_mask(table, s_total):
    m = torch.zeros(s_total, dtype=torch.bool)
    for off, ln in table:
        m[off:off + ln] = True
    return m


@functools.lru_cache(maxsize=None)
def _operands(name):
    """host operands of a table in the packed layouts: NaN sentinels (q, v_rm, dO) / the largest finite bf16 (caches) outside the sequences"""
    nh, table = TABLES[name]
    s_total, smax = _geometry(table)
    g = _gen(len(table), nh, s_total, 41)
    rows = _row_mask(table, s_total)
    q = _bf_sentinel((nh, s_total, HD))
    v_rm = _bf_sentinel((nh, s_total, HD))
    do_hm = _bf_sentinel((nh, s_total, HD))
    kc = R.garbage((nh, smax, HD))
    vt = R.garbage((nh, HD, smax))
    n = int(rows.sum())
    q[:, rows] = (torch.randn(nh, n, HD, generator=g) * 1.5).bfloat16()
    kc[:, :s_total][:, rows] = (torch.randn(nh, n, HD, generator=g) * 1.5).bfloat16()
    v = torch.randn(nh, n, HD, generator=g).bfloat16()
    v_rm[:, rows] = v
    vt[:, :, :s_total][:, :, rows] = v.transpose(1, 2)
    do_hm[:, rows] = torch.randn(nh, n, HD, generator=g).bfloat16()
    ld_do = nh * HD + 8                                              # token-major dO with a row pitch of its own
    do_tm = _bf_sentinel((s_total, ld_do))
    do_tm[rows, :nh * HD] = do_hm[:, rows].permute(1, 0, 2).reshape(n, nh * HD)
    return dict(nh=nh, table=table, s_total=s_total, smax=smax, rows=rows, q=q, kc=kc, vt=vt, v_rm=v_rm, do_hm=do_hm, do_tm=do_tm, ld_do=ld_do)


def _launch_all(D, table, max_len, o_lse=None, raw=False):
    """the three variable-length entry points on the operands ``D`` with ``table``; returns the slabs.  ``raw``: straight to the C entry
    points (no host check of the table).  ``o_lse``: (o, lse) host tensors the backward is given instead of this forward's outputs."""
    ops, L = _ops(), _lib()
    nh, s_total, smax = D["nh"], D["s_total"], D["smax"]
    sp = SPARE * nh * HD
    S = {k: _Slab(D[k].shape, BF, 3 * sp if k == "do_tm" else sp, D[k]) for k in ("q", "kc", "vt", "v_rm", "do_hm", "do_tm")}
    S["out"] = _Slab((s_total, nh * HD), BF, sp)
    S["lse"] = _Slab((nh, s_total), F32, SPARE)
    seqs = torch.tensor(table, dtype=torch.int32).to(DEV)
    nseq = len(table)
    cos, sin = (t.to(DEV) for t in R.rope_tables(MAX_POS))
    if raw:
        rc = L.llark_attn_prefill_bf16_lse_varlen(S["q"].view.data_ptr(), S["kc"].view.data_ptr(), S["vt"].view.data_ptr(), seqs.data_ptr(), nseq, max_len,
                                                  s_total, nh, HD, smax, S["out"].view.data_ptr(), S["lse"].view.data_ptr(), _stream())
        assert rc == 0
    else:
        ops.attn_prefill_lse_varlen(S["q"].view, S["kc"].view, S["vt"].view, seqs, table, max_len, s_total, nh, HD, S["out"].view, S["lse"].view)
    torch.cuda.synchronize()
    if o_lse is None:
        S["o_in"], S["lse_in"] = _Slab(S["out"].shape, BF, sp, S["out"].view.cpu()), _Slab(S["lse"].shape, F32, SPARE, S["lse"].view.cpu())
    else:
        S["o_in"], S["lse_in"] = _Slab(S["out"].shape, BF, sp, o_lse[0]), _Slab(S["lse"].shape, F32, SPARE, o_lse[1])
    for k in ("dsum", "dsum_f"):
        S[k] = _Slab((nh, s_total), F32, SPARE)
    for k in ("dq", "dk", "dv"):
        S[k] = _Slab((nh, s_total, HD), F32, sp)
    S["dqkv"] = _Slab((s_total, 3 * nh * HD), BF, 3 * sp)
    if raw:
        p = {k: v.view.data_ptr() for k, v in S.items()}
        rc = L.llark_attn_backward_bf16_varlen(p["q"], p["kc"], p["v_rm"], p["do_hm"], p["o_in"], p["lse_in"], p["dsum"], seqs.data_ptr(), nseq, max_len,
                                               s_total, nh, HD, smax, p["dq"], p["dk"], p["dv"], _stream())
        assert rc == 0
        rc = L.llark_attn_backward_bf16_fused_varlen(p["q"], p["kc"], p["v_rm"], p["do_tm"], D["ld_do"], p["o_in"], p["lse_in"], p["dsum_f"], seqs.data_ptr(),
                                                     nseq, max_len, s_total, nh, HD, smax, cos.data_ptr(), sin.data_ptr(), MAX_POS, p["dqkv"], _stream())
        assert rc == 0
    else:
        ops.attn_backward_varlen(S["q"].view, S["kc"].view, S["v_rm"].view, S["do_hm"].view, S["o_in"].view, S["lse_in"].view, S["dsum"].view, seqs, table,
                                 max_len, s_total, nh, HD, S["dq"].view, S["dk"].view, S["dv"].view)
        ops.attn_backward_fused_varlen(S["q"].view, S["kc"].view, S["v_rm"].view, S["do_tm"].view, S["o_in"].view, S["lse_in"].view, S["dsum_f"].view, seqs,
                                       table, max_len, s_total, nh, HD, cos, sin, S["dqkv"].view)
    torch.cuda.synchronize()
    return S


OUTPUTS = ("out", "lse", "dsum", "dsum_f", "dq", "dk", "dv", "dqkv")


def _results(D, S, table):
    """host copies of every output after the untouched-outside-the-sequences check; inputs bit-unchanged"""
    nh, s_total = D["nh"], D["s_total"]
    rows = _row_mask(table, s_total)
    written = {"out": rows[:, None].expand(s_total, nh * HD), "lse": rows[None, :].expand(nh, s_total),
               "dq": rows[None, :, None].expand(nh, s_total, HD), "dqkv": rows[:, None].expand(s_total, 3 * nh * HD)}
    written.update(dsum=written["lse"], dsum_f=written["lse"], dk=written["dq"], dv=written["dq"])
    got = {k: S[k].result(k, written[k]) for k in OUTPUTS}
    for k in ("q", "kc", "vt", "v_rm", "do_hm", "do_tm", "o_in", "lse_in"):
        S[k].unchanged(k)
    return got


def _uniform(D, off, ln, o_b=None, lse_b=None):
    """the uniform entry points with batch = 1, s = ln on copies of the rows off .. off + ln - 1: dict of host results"""
    ops = _ops()
    nh = D["nh"]
    smax_b = R.round_up(ln, 8) + 8
    sl = slice(off, off + ln)
    q = D["q"][:, sl].contiguous().to(DEV)
    kc = R.k_cache(D["kc"][:, sl].contiguous(), 1, nh, smax_b).to(DEV)
    vt = R.vt_cache(D["v_rm"][:, sl].contiguous(), 1, nh, smax_b).to(DEV)
    v_rm = D["v_rm"][:, sl].contiguous().to(DEV)
    do_hm = D["do_hm"][:, sl].contiguous().to(DEV)
    do_tm = D["do_tm"][sl].contiguous().to(DEV)
    out = torch.empty(ln, nh * HD, dtype=BF, device=DEV)
    lse = torch.empty(nh, ln, dtype=F32, device=DEV)
    ops.attn_prefill_lse(q.view(1, nh, ln, HD), kc, vt, 1, ln, nh, HD, out, lse)
    o_in = out if o_b is None else o_b.contiguous().to(DEV)
    lse_in = lse if lse_b is None else lse_b.contiguous().to(DEV)
    dsum, dsum_f = torch.empty_like(lse), torch.empty_like(lse)
    dq, dk, dv = (torch.empty(nh, ln, HD, dtype=F32, device=DEV) for _ in range(3))
    ops.attn_backward(q, kc, v_rm, do_hm, o_in, lse_in, dsum, 1, ln, nh, HD, dq, dk, dv)
    dqkv = torch.empty(ln, 3 * nh * HD, dtype=BF, device=DEV)
    cos, sin = (t.to(DEV) for t in R.rope_tables(MAX_POS))
    ops.attn_backward_fused(q, kc, v_rm, do_tm, o_in, lse_in, dsum_f, 1, ln, nh, HD, cos, sin, 0, dqkv)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(out=out, lse=lse, dsum=dsum, dsum_f=dsum_f, dq=dq, dk=dk, dv=dv, dqkv=dqkv).items()}


def _slice_of(name, t, off, ln):
    """rows off .. off + ln - 1 of packed output ``name``"""
    if name in ("out", "dqkv"):
        return t[off:off + ln]
    return t[:, off:off + ln]


def _assert_bit_equal(tag, got, D, table):
    for b, (off, ln) in enumerate(table):
        ref = _uniform(D, off, ln, _slice_of("out", got["out"], off, ln), _slice_of("lse", got["lse"], off, ln))
        for k in OUTPUTS:
            a, r = _bits(_slice_of(k, got[k], off, ln).contiguous()), _bits(ref[k])
            assert torch.equal(a, r), f"{tag}: {k} of sequence {b} (off {off}, len {ln}): {int((a != r).sum())} of {a.numel()} elements differ from the uniform call"


@pytest.mark.parametrize("name", list(TABLES))
def test_varlen_bit_equal_to_uniform_per_sequence(name):
    """a base offset of the wrong plane or stride, a tile count taken from max_len, a pair index that escapes its sequence, a block
    numbering that hands a (sequence, head) to the wrong workgroup, a RoPE position taken from the global row, a row outside a sequence
    read or written"""
    D = _operands(name)
    table = D["table"]
    max_len = max(n for _, n in table)
    S = _launch_all(D, table, max_len)
    got = _results(D, S, table)
    for k in OUTPUTS:
        sel = _slice_of(k, got[k], 0, D["s_total"])
        inside = sel[D["rows"]] if k in ("out", "dqkv") else sel[:, D["rows"]]
        assert not bool(torch.isnan(inside.float()).any()), f"{k}: a sentinel inside a sequence"
    _assert_bit_equal(name, got, D, table)
    # a second launch repeats the first bit for bit (the backward on the same o / lse)
    again = _results(D, _launch_all(D, table, max_len), table)
    for k in OUTPUTS:
        assert torch.equal(_bits(again[k]), _bits(got[k])), f"{k}: the second launch differs from the first"
    # a max_len above every length only adds workgroups that return
    wide = _results(D, _launch_all(D, table, min(D["s_total"], max_len + 70)), table)
    for k in OUTPUTS:
        assert torch.equal(_bits(wide[k]), _bits(got[k])), f"{k}: differs with a larger max_len"


def test_varlen_forward_against_float64():
    """the forward of the first table under the bounds of test_llama_kernels_gpu.py, sequence by sequence"""
    D = _operands("tiles")
    table, nh = D["table"], D["nh"]
    S = _launch_all(D, table, max(n for _, n in table))
    got = _results(D, S, table)
    for b, (off, ln) in enumerate(table):
        sl = slice(off, off + ln)
        ref = R.reference(D["q"][:, sl].double(), D["kc"][:, sl].double(), D["v_rm"][:, sl].double(), 0)
        R.check_out(f"varlen out, sequence {b}", "lse", R.from_rows(got["out"][sl].double(), 1, nh), ref)
        R.check_lse(f"varlen lse, sequence {b}", got["lse"][:, sl].double(), ref)


def test_varlen_scalar_declines_before_any_launch():
    L = _lib()
    x = torch.zeros(64, device=DEV)                                     # any valid device pointer: nothing is launched
    p, st = x.data_ptr(), _stream()

    def fwd(q=p, seqs=p, nseq=1, max_len=8, s_total=8, nh=2, hd=HD, smax=8):
        return L.llark_attn_prefill_bf16_lse_varlen(q, p, p, seqs, nseq, max_len, s_total, nh, hd, smax, p, p, st)

    def bwd(q=p, seqs=p, nseq=1, max_len=8, s_total=8, nh=2, hd=HD, smax=8):
        return L.llark_attn_backward_bf16_varlen(q, p, p, p, p, p, p, seqs, nseq, max_len, s_total, nh, hd, smax, p, p, p, st)

    def fused(q=p, seqs=p, nseq=1, max_len=8, s_total=8, nh=2, hd=HD, smax=8, max_pos=MAX_POS):
        return L.llark_attn_backward_bf16_fused_varlen(q, p, p, p, 2 * HD, p, p, p, seqs, nseq, max_len, s_total, nh, hd, smax, p, p, max_pos, p, st)

    for name, f in (("attn_prefill_lse_varlen", fwd), ("attn_backward_varlen", bwd), ("attn_backward_fused_varlen", fused)):
        for what, kw in (("head_dim", dict(hd=64)), ("bad shape", dict(smax=12, s_total=8)), ("bad shape", dict(s_total=16, smax=8)),
                         ("bad shape", dict(max_len=16)), ("bad shape", dict(nseq=0)), ("null pointer", dict(q=None)), ("null pointer", dict(seqs=None))):
            assert f(**kw) == ERR_INVALID, (name, kw)
            msg = L.llark_last_error().decode()
            assert msg.startswith(name + ":") and what in msg, (name, kw, msg)
    assert fused(max_len=8, max_pos=4) == ERR_INVALID and "RoPE table" in L.llark_last_error().decode()
    torch.cuda.synchronize()
    assert bool((x == 0).all())


def test_varlen_wrappers_name_the_table_rule():
    ops = _ops()
    D = _operands("gaps")
    nh, s_total = D["nh"], D["s_total"]
    for table, max_len, says in (([(4, 8)], 8, "off % 8"), ([(0, 16), (8, 16)], 16, "disjoint"), ([(16, 8), (0, 24)], 24, "disjoint"),
                                 ([(s_total - 8, 16)], 16, "off + len <= s_total"), ([(0, 16), (16, 24)], 16, "max_len >= max"),
                                 ([(0, 0)], 8, "len >= 1"), ([], 8, "empty")):
        for call in ("fwd", "bwd", "fused"):
            with pytest.raises(ValueError, match=re.escape(says)):
                ops.check_seq_table(table, max_len, s_total)
            seqs = torch.zeros((max(len(table), 1), 2), dtype=torch.int32, device=DEV)
            t = torch.zeros(8, device=DEV)
            with pytest.raises(ValueError, match=re.escape(says)):
                if call == "fwd":
                    ops.attn_prefill_lse_varlen(t, t, t, seqs, table, max_len, s_total, nh, HD, t, t)
                elif call == "bwd":
                    ops.attn_backward_varlen(t, t, t, t, t, t, t, seqs, table, max_len, s_total, nh, HD, t, t, t)
                else:
                    ops.attn_backward_fused_varlen(t, t, t, t, t, t, t, seqs, table, max_len, s_total, nh, HD, t, t, t)


def test_varlen_malformed_table_entries_touch_nothing():
    """entries that break a rule, straight to the C entry points: the guard is seen by its effect on memory -- nothing of theirs is
    written, the well-formed neighbours are computed as ever.  Every tensor has SPARE rows behind it, so even the entry that runs past
    s_total lies inside the allocations."""
    D = _operands("tiles")
    s_total = D["s_total"]
    good = [(0, 64), (72, 136)]
    bad = [(64, 0), (s_total - 8, 8 + SPARE // 2), (212, 8)]                          # len 0; beyond s_total; off % 8
    table = [good[0], bad[0], bad[1], good[1], bad[2]]
    # o / lse of the backward: finite everywhere, so that a bad entry's rows would be computed (and seen) if its guard failed
    ok = _results(D, _launch_all(D, D["table"], 136), D["table"])
    S = _launch_all(D, table, 64 + 70, o_lse=(ok["out"], ok["lse"]), raw=True)        # len 136 > max_len 134: the second good entry is refused too
    got = _results(D, S, [good[0]])
    _assert_bit_equal("malformed", got, D, [good[0]])
    S = _launch_all(D, table, 136, o_lse=(ok["out"], ok["lse"]), raw=True)
    got = _results(D, S, good)
    _assert_bit_equal("malformed", got, D, good)
