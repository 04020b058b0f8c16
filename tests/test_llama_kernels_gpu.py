"""The Llama inference kernels of csrc/llama.hip -- attn_prefill_kernel, attn_decode_kernel, rope_split_kernel, rmsnorm_kernel,
embed_gather_kernel -- one kernel at a time against the float64 references of tests/llama_kernel_ref.py.

Every output element is compared with the reference under a bound made of the documented roundings of the kernel (below); every
output buffer lies in a sentinel slab that is asserted bit-unchanged around the output; every input is asserted bit-unchanged (for
the fused decode forms: everything except the appended K row and V^T column, which must be bit-equal to torch's float32
``q1 * c + (-q2) * s`` rounded the same way).  The attention operands carry PLANTED keys (``k_j += 0.6 q_i``: probability ~0.9) on
the diagonal of the first, 16th, 17th and last query of every query set and of the ragged last block, at keys 63 | 64, key 0, the
first key of the ragged tile and the last key -- losing, doubling or misplacing one moves all 128 outputs of a query by O(1) -- and
on the first MASKED key of a few queries, which must not show.  Cache positions >= total hold the largest finite bf16 (0x7F7F) in
every plane, not zeros: a key read past ``total`` is seen.  tests/test_llama_kernel_ref_cpu.py shows on the CPU that these bounds
reject such defects and accept the correct arithmetic.

Tolerances (``B = sum_j p_j |v_jd|``, ``A = max_j (scale sum_d |q_d k_jd| + |alibi_j|)``; ``u`` = one bf16 ulp of the reference for one
output plane, 2^-16 |ref| for hi + lo planes; ``c = max(16, 4 r)``, ``r`` = torch's own float32 CPU result of the same operation on the
same operands, in units of 2^-24 (1 + 2A) B, measured inside each test):

    output                                  tolerance                                      format coefficient from
    decode, all forms                       u + c 2^-24 (1 + 2A) B                         fp32 only (fma chains, expf)
    prefill, bf16 operands (P2)             u + (2^-16 + c 2^-24 (1 + 2A)) B               p as bf16 hi + lo
    prefill, hi + lo operands (SPLIT)       u + (2^-16 (2 + 2A) + c 2^-24 (1 + 2A)) B      + the two dropped lo.lo products
    prefill _lse                            u + (2^-8 + c 2^-24 (1 + 2A)) B                p rounded to bf16 once
    lse                                     c 2^-24 (1 + |lse| + A)                        fp32 only
    RoPE q, k: hi + lo                      2^-16 |ref| + 4 2^-24 (|x1 c| + |x2 s|)        (hi alone: one bf16 ulp + the same)
    RMSNorm                                 u + c 2^-24 |w| |x| rstd                       c from torch float32
    V planes, embedding gather              bit-exact

Measured: worst torch float32 ratio ``r`` (units of 2^-24 times the fp32 bound) and the kernels' worst error as a FRACTION OF THE
TOLERANCE on the MI355X, over the cases of this file (``-s`` prints each case's own figures as "[ratio] ..."):

    output                                  r (torch fp32)   kernel / tolerance
    decode bf16 out, 16 waves               1.63             0.98
    decode bf16 out, 4 waves                1.99             0.98
    decode split out, 16 waves              3.24             0.14
    decode split out, 4 waves               3.31             0.15
    decode out, mixed rows (bf16 | split)   2.07             0.98
    prefill bf16 out, NQ = 1                1.38             0.98
    prefill bf16 out, NQ = 2                1.86             0.98
    prefill split out (NQ = 1)              3.56             0.05
    prefill _lse out, NQ = 1                1.38             0.86
    prefill _lse out, NQ = 2                1.86             0.90
    lse, NQ = 1                             2.47             0.12
    lse, NQ = 2                             2.83             0.12
    RoPE q | k, hi                          -                1.00 | 0.99       (the kernel's float32 expression is also bit-equal to torch's)
    RoPE q | k, hi + lo                     -                0.49 | 0.49
    RMSNorm hi                              3.37             0.99
    RMSNorm hi + lo                         3.37             0.47

``c`` was 16 in every case (r < 4).  A single bf16 output plane sits at 0.98 .. 1.00 of its tolerance by construction: round to nearest
errs by up to half an ulp, which is 2^-8 |ref| -- the whole of ``u`` -- just above a power of two; what the kernel's own arithmetic adds
shows in the hi + lo rows.  The whole file: 137 cases in 34 s on the MI355X.

Prefill case ids name the instantiation attn_prefill_kernel<SPLIT, NQ, P2, ALIBI>, paired or single query blocks, the block count
and the block numbering (``xcd``: batch * nh % 8 == 0) the launcher's rule picks for the shape; llama_kernel_ref.prefill_rule restates
that rule and the CPU file pins it for every shape.  Paired grids with batch * nh % 8 != 0 need sequences of several thousand
positions and are left out.  Decode case ids name the wave count of attn_decode_kernel<NW, UBT>.

These tests are why the V pass of attn_decode_kernel leaves the columns total .. round_up(total, 8) - 1 of hi + lo caches out of
its sum instead of multiplying them by p = 0: float(hi) + float(lo) of two stale planes can overflow (0x7F7F + 0x7F7F = inf), and
0 * inf turned every output of the head into NaN whenever total % 8 != 0 (measured with the former kernel: all 256 outputs of the
1 x 2 hi + lo case non-finite at total = 1; the bf16 cases pass either way); and why attn_decode() refuses smax % 8 != 0 for the
unfused forms too.  Pairs of planes written by store_split never overflow that way (|lo| <= 2^-9 |hi|), so no engine state changes
its result; the extra branch costs the 64-token generate benchmark 0.45 % (3.298 against 3.313 clips/s, two alternating runs each).
"""
import functools

import numpy as np
import pytest
import torch

import llama_kernel_ref as R
from kernel_util import EPS24, assert_untouched as _assert_untouched, bf16_ulp as _bf16_ulp, bf_sentinel as _bf_sentinel, bits as _bits, \
    check_frac as _check_frac, gen as _gen, out_slab as _out_slab, tol as _tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = R.HD
BF = torch.bfloat16
PAD = 8                                           # elements in front of an output inside its slab: keeps the 16-byte alignment of the planes
ERR_INVALID, ERR_UNSUPPORTED = -1, -2             # include/llark_hip.h


def _ops():
    from llark_amd import ops
    return ops


def _lib():
    from llark_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _same(name, dev_t, host_t):
    assert torch.equal(_bits(dev_t), _bits(host_t)), f"{name}: an input was modified"


def _same_dev(name, a, b):
    """bit equality of two device tensors, compared on the device"""
    w = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.view(w), b.view(w)), f"{name}: {int((a.view(w) != b.view(w)).sum())} elements differ"


class _Out:
    """an output of ``n`` elements inside a sentinel slab on the device"""

    def __init__(self, n, dtype=BF):
        self.host, self.mask = _out_slab(n, dtype, front=PAD, back=PAD)
        self.dev = self.host.to(DEV)
        self.view = self.dev[PAD:PAD + n]

    def result(self, name, written=None):
        """the output on the host, after asserting that nothing around it (or outside ``written``) was touched"""
        _assert_untouched(name, self.dev, self.host, self.mask if written is None else written)
        return self.dev.cpu()[PAD:PAD + int(self.mask.sum())]


# =====================================================================================================================
# 1. prefill: attn_prefill_kernel<SPLIT, NQ, P2, ALIBI>
# =====================================================================================================================
def _prefill_cases():
    cases = []
    for shape in R.PREFILL_SHAPES:
        for alibi in (False, True):
            if alibi and shape not in R.PREFILL_ALIBI:
                continue
            for mode in ("bf16", "lse", "split"):          # bf16 and lse share operands and reference
                if (mode == "lse" and shape[3] != 0) or (mode == "split" and shape in R.PREFILL_SPLIT_DROPPED):
                    continue
                cases.append(pytest.param(shape, mode, alibi, id=R.prefill_case_id(shape, mode, alibi)))
    return cases


@functools.lru_cache(maxsize=1)
def _prefill_ref(shape, split, alibi):
    batch, nh, s, past = shape
    o = R.prefill_operands(batch, nh, s, past, split)
    slopes = R.alibi_slopes(nh) if alibi else None
    sl_n = None if slopes is None else slopes.double().repeat(batch)
    ref = R.reference(R.value(*o["q"]), R.value(*o["k"]), R.value(*o["v"]), past, sl_n)
    return o, slopes, ref


@pytest.mark.parametrize("shape,mode,alibi", _prefill_cases())
def test_attn_prefill(shape, mode, alibi):
    """a causal mask one key early or late, a `total` clamp off by one in the ragged last tile, a tile or query set handed to the
    wrong wave or workgroup (paired blocks, XCD numbering), a key read past `total`, a probability plane dropped"""
    ops = _ops()
    batch, nh, s, past = shape
    split = mode == "split"
    total, N = past + s, batch * nh
    o, slopes, ref = _prefill_ref(shape, split, alibi)
    smax = R.round_up(total, 8) + 8
    host = {"q": [None if p is None else p.view(batch, nh, s, HD) for p in o["q"]],
            "k": [None if p is None else R.k_cache(p, batch, nh, smax) for p in o["k"]],
            "v": [None if p is None else R.vt_cache(p, batch, nh, smax) for p in o["v"]]}
    dev = {n: [None if p is None else p.to(DEV) for p in ps] for n, ps in host.items()}
    d_slopes = None if slopes is None else slopes.to(DEV)
    out = _Out(batch * s * nh * HD)
    out_lo = _Out(batch * s * nh * HD) if split else None
    lse = _Out(N * s, torch.float32) if mode == "lse" else None
    shape2 = (batch * s, nh * HD)
    if mode == "lse":
        ops.attn_prefill_lse(dev["q"][0], dev["k"][0], dev["v"][0], batch, s, nh, HD, out.view.view(shape2), lse.view.view(N, s), alibi_slopes=d_slopes)
    elif split:
        ops.attn_prefill(dev["q"][0], dev["k"][0], dev["v"][0], batch, s, nh, HD, past, out.view.view(shape2), dev["q"][1], dev["k"][1], dev["v"][1],
                         out_lo.view.view(shape2), alibi_slopes=d_slopes)
    else:
        ops.attn_prefill(dev["q"][0], dev["k"][0], dev["v"][0], batch, s, nh, HD, past, out.view.view(shape2), alibi_slopes=d_slopes)
    _sync()
    for n in "qkv":
        for i, p in enumerate(dev[n]):
            if p is not None:
                _same(f"{n} plane {i}", p, host[n][i])
    got = out.result("out").view(shape2).double()
    if split:
        got = got + out_lo.result("out_lo").view(shape2).double()
    name = R.prefill_case_id(shape, mode, alibi)
    R.check_out(f"prefill {name}", mode, R.from_rows(got, batch, nh), ref)
    if mode == "lse":
        R.check_lse(f"prefill lse {name}", lse.result("lse").view(N, s).double(), ref)


# =====================================================================================================================
# 2. decode: attn_decode_kernel<16, 4> / <4, 8>, six forms
# =====================================================================================================================
SMAX = 520
TOTALS = [1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257, 371, 513]
DECODE_GRIDS = [(1, 2), (3, 32), (8, 32), (16, 32)]
DECODE_CASES = [(b, h, split, False) for b, h in DECODE_GRIDS for split in (False, True)] + [(3, 32, True, True), (8, 32, False, True)]


def _decode_id(batch, nh, split, alibi):
    return f"{'split' if split else 'bf16'}{'_alibi' if alibi else ''}-{batch}x{nh}-<{R.decode_waves(batch, nh)},{4 if R.decode_waves(batch, nh) == 16 else 8}>"


class _Decode:
    """seeded caches of SMAX positions for (batch, nh): the K / V^T planes on the device, the operand values on the host"""

    def __init__(self, batch, nh, split, alibi):
        self.batch, self.nh, self.split, self.N = batch, nh, split, batch * nh
        g = _gen(batch, nh, 911)
        N = self.N
        self.kb = torch.randn(N, SMAX, HD, generator=g) * 1.5          # keys BEFORE the rotation for the row a step appends, after it elsewhere
        self.vb = torch.randn(N, SMAX, HD, generator=g)
        self.qraw = torch.randn(N, HD, generator=g) * 1.5              # the new token's q before the rotation
        cut = R.planes if split else (lambda x: (x.bfloat16(), None))
        self.cut = cut
        self.kp, self.vp = cut(self.kb), cut(self.vb)
        self.k64, self.v64 = R.value(*self.kp), R.value(*self.vp)
        self.d_k = [None if p is None else p.to(DEV).view(batch, nh, SMAX, HD) for p in self.kp]
        self.d_vt = [None if p is None else p.to(DEV).view(batch, nh, SMAX, HD).transpose(2, 3).contiguous() for p in self.vp]
        self.cos, self.sin = R.rope_tables(SMAX)
        self.d_cos, self.d_sin = self.cos.to(DEV), self.sin.to(DEV)
        self.slopes = R.alibi_slopes(nh) if alibi else None
        self.d_slopes = None if self.slopes is None else self.slopes.to(DEV)

    def state(self, pos_rows, smax, refs=None):
        """The step that appends position pos_rows[b] to sequence b (idle: < 0 or >= smax).  Returns the caches on the device
        AFTER the step (`final`) and before it (`pre`: the appended row / column still garbage), the q planes, the raw qkv, and
        per distinct position the float64 reference of its rows."""
        batch, nh, N = self.batch, self.nh, self.N
        live = [b for b in range(batch) if 0 <= pos_rows[b] < smax]
        cf = torch.contiguous_format                                   # (copies: the seed planes stay as they are)
        k_fin = [None if p is None else p[:, :, :smax].clone(memory_format=cf) for p in self.d_k]
        vt_fin = [None if p is None else p[:, :, :, :smax].clone(memory_format=cf) for p in self.d_vt]
        gar = R.garbage((1,)).to(DEV)
        qrot = torch.zeros(N, HD)
        kraw = torch.zeros(N, HD)
        patches = {}
        for b in range(batch):
            sl = slice(b * nh, (b + 1) * nh)
            if b not in live:                                          # an idle slot keeps whatever it held: all SMAX positions of the seed
                continue
            pos = pos_rows[b]
            total = pos + 1
            c, s = self.cos[pos], self.sin[pos]
            qrot[sl] = R.rope(self.qraw[sl], c, s, torch.float32)
            kraw[sl] = self.kb[sl, pos] + R.PLANT * self.qraw[sl]      # planted before the rotation: the rotation is linear
            rows = {pos: R.rope(kraw[sl], c, s, torch.float32)}
            for j in R.decode_plants(total):
                if j != pos:
                    rows[j] = self.kb[sl, j] + R.PLANT * qrot[sl]
            patches[b] = {j: self.cut(x) for j, x in rows.items()}
            for j, pl in patches[b].items():
                for i, p in enumerate(pl):
                    if p is not None:
                        k_fin[i][b, :, j] = p.to(DEV)
            for i in range(len(k_fin)):
                if k_fin[i] is not None:
                    k_fin[i][b, :, total:] = gar
                    vt_fin[i][b, :, :, total:] = gar
        k_pre = [None if p is None else p.clone() for p in k_fin]
        vt_pre = [None if p is None else p.clone() for p in vt_fin]
        for b in live:
            for i in range(len(k_pre)):
                if k_pre[i] is not None:
                    k_pre[i][b, :, pos_rows[b]] = gar
                    vt_pre[i][b, :, :, pos_rows[b]] = gar
        qp = self.cut(qrot)
        q64 = R.value(*qp)
        qkv = torch.cat((self.qraw.view(batch, nh * HD), kraw.view(batch, nh * HD),
                         torch.stack([self.vb[b * nh:(b + 1) * nh, max(0, min(pos_rows[b], SMAX - 1))] for b in range(batch)]).view(batch, nh * HD)), dim=1)
        have, refs = refs is not None, ([] if refs is None else refs)       # (a reference does not depend on smax: the caller may hand it back)
        for pos in ([] if have else sorted({pos_rows[b] for b in live})):
            grp = [b for b in live if pos_rows[b] == pos]
            n_idx = torch.cat([torch.arange(b * nh, (b + 1) * nh) for b in grp])
            total = pos + 1
            k = self.k64[n_idx, :total].clone() if len(grp) < batch else self.k64[:, :total]
            saved = {}
            for gi, b in enumerate(grp):
                for j, pl in patches[b].items():
                    saved[(gi, j)] = k[gi * nh:(gi + 1) * nh, j].clone()
                    k[gi * nh:(gi + 1) * nh, j] = R.value(*pl)
            sl_n = None if self.slopes is None else self.slopes.double().repeat(len(grp))
            ref = R.reference(q64[n_idx][:, None, :], k, self.v64[n_idx, :total] if len(grp) < batch else self.v64[:, :total], pos, sl_n)
            for (gi, j), x in saved.items():
                k[gi * nh:(gi + 1) * nh, j] = x
            refs.append((grp, ref))
        return dict(k_fin=k_fin, vt_fin=vt_fin, k_pre=k_pre, vt_pre=vt_pre, q=[None if p is None else p.view(batch, nh, HD).to(DEV) for p in qp],
                    qkv=qkv.contiguous(), refs=refs, live=live)


@functools.lru_cache(maxsize=1)
def _decode_data(batch, nh, split, alibi):
    return _Decode(batch, nh, split, alibi)


def _check_decode(name, D, st, out, out_lo):
    batch, nh = D.batch, D.nh
    got = out.result(f"{name} out").view(batch, nh, HD).double()
    if D.split:
        got = got + out_lo.result(f"{name} out_lo").view(batch, nh, HD).double()
    for grp, ref in st["refs"]:
        g = torch.cat([got[b] for b in grp])[:, None, :]
        R.check_out(f"{name} rows {grp[0]}..", "decode_split" if D.split else "decode", g, ref)
    for b in range(batch):
        if b not in st["live"]:
            assert bool((got[b] == 0).all()), f"{name}: idle row {b} is not zero"


def _run_forms(D, st, pos, smax, tag, forms):
    """every decode form on the same step; `pos` None: rows form only (mixed positions, given in st)"""
    ops = _ops()
    batch, nh, split = D.batch, D.nh, D.split
    n_out = batch * nh * HD
    lo = (lambda ps: ps[1]) if split else (lambda ps: None)
    d_qkv = st["qkv"].to(DEV)
    for form in forms:
        name = f"{tag} {form}"
        out, out_lo = _Out(n_out), (_Out(n_out) if split else None)
        o2, ol2 = out.view.view(batch, nh * HD), (out_lo.view.view(batch, nh * HD) if split else None)
        if form in ("host", "dpos"):
            k, vt = [None if p is None else p.clone() for p in st["k_fin"]], [None if p is None else p.clone() for p in st["vt_fin"]]
            q = [None if p is None else p.clone() for p in st["q"]]
            if form == "host":
                ops.attn_decode(q[0], k[0], vt[0], batch, nh, HD, pos + 1, o2, lo(q), lo(k), lo(vt), ol2, alibi_slopes=D.d_slopes)
            else:
                if D.d_slopes is not None:                             # llark_attn_decode_bf16_dpos takes no ALiBi
                    continue
                ops.attn_decode_dpos(q[0], k[0], vt[0], batch, nh, HD, torch.tensor([pos], dtype=torch.int32, device=DEV), o2, lo(q), lo(k), lo(vt), ol2)
            _sync()
            for i in range(len(q)):
                if q[i] is not None:
                    _same_dev(f"{name} q plane {i}", q[i], st["q"][i])
        else:
            k, vt = [None if p is None else p.clone() for p in st["k_pre"]], [None if p is None else p.clone() for p in st["vt_pre"]]
            qkv = d_qkv.clone()
            if form == "rope_host":
                ops.attn_decode_rope(qkv, batch, nh, HD, pos, D.d_cos, D.d_sin, k[0], vt[0], o2, lo(k), lo(vt), ol2, alibi_slopes=D.d_slopes)
            elif form == "rope_dpos":
                ops.attn_decode_rope(qkv, batch, nh, HD, torch.tensor([pos], dtype=torch.int32, device=DEV), D.d_cos, D.d_sin, k[0], vt[0], o2, lo(k), lo(vt), ol2,
                                     alibi_slopes=D.d_slopes)
            elif form == "rows":
                rows = torch.tensor(st["pos_rows"], dtype=torch.int32, device=DEV)
                ops.attn_decode_rope_rows(qkv, batch, nh, HD, rows, D.d_cos, D.d_sin, k[0], vt[0], o2, lo(k), lo(vt), ol2, alibi_slopes=D.d_slopes)
            else:
                if D.d_slopes is not None:                             # the chained binding passes no ALiBi
                    continue
                done = torch.zeros(4, dtype=torch.int32, device=DEV)
                ops.attn_decode_rope_chain(qkv, batch, nh, HD, pos, D.d_cos, D.d_sin, k[0], vt[0], o2, lo(k), lo(vt), ol2, done)
                _sync()
                assert done.cpu().tolist() == [nh * batch, 0, 0, 0], f"{name}: arrival counter {done.cpu().tolist()}"
            _sync()
            _same_dev(f"{name} qkv", qkv, d_qkv)
        # unfused: the caches are inputs.  fused: the appended row / column must be bit-equal to torch's float32 rotation rounded to
        # the planes, and everything else -- the garbage beyond `total` included -- untouched: both are `equal to the final state`
        for i in range(len(k)):
            if k[i] is not None:
                _same_dev(f"{name} k cache plane {i}", k[i], st["k_fin"][i])
                _same_dev(f"{name} v^T cache plane {i}", vt[i], st["vt_fin"][i])
        _check_decode(name, D, st, out, out_lo)


FORMS = ["host", "dpos", "rope_host", "rope_dpos", "rows", "chain"]


@pytest.fixture(scope="module", autouse=True)
def _release_shared_data():
    yield
    _prefill_ref.cache_clear()
    _decode_data.cache_clear()


@pytest.mark.parametrize("batch,nh,split,alibi", [pytest.param(*c, id=_decode_id(*c)) for c in DECODE_CASES])
def test_attn_decode(batch, nh, split, alibi):
    """a key lost or read twice at a round boundary of the K pass (128 keys at 4 waves, 256 at 16) or of the 8-key V chunks, a
    clamped re-load that is not skipped, a key read past `total` (the garbage), the fused append writing the wrong row or plane,
    the arrival counter of the chained form"""
    D = _decode_data(batch, nh, split, alibi)
    for total in TOTALS:
        refs = None
        for smax in sorted({R.round_up(total, 8), SMAX}):
            st = D.state([total - 1] * batch, smax, refs)
            refs = st["refs"]
            st["pos_rows"] = [total - 1] * batch
            _run_forms(D, st, total - 1, smax, f"decode {_decode_id(batch, nh, split, alibi)} total={total} smax={smax}", FORMS)


ROWS_CASES = {(3, 32): [[256, -1, 8], [519, 520, 0]], (8, 32): [[0, 7, -1, 127, 128, 600, 370, 512]],
              (16, 32): [[t - 1 for t in TOTALS] + [-1, SMAX, 254]]}


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("batch,nh", list(ROWS_CASES), ids=lambda v: str(v))
def test_attn_decode_rows_mixed(batch, nh, split):
    """one position per sequence: a row using another row's position or cache slot, an idle row (-1, or a position >= smax) that
    writes to its caches or leaves its output head unwritten"""
    D = _decode_data(batch, nh, split, False)
    for pos_rows in ROWS_CASES[(batch, nh)]:
        st = D.state(pos_rows, SMAX)
        st["pos_rows"] = pos_rows
        _run_forms(D, st, None, SMAX, f"decode rows {batch}x{nh} {pos_rows}", ["rows"])


def test_attn_decode_refuses_smax_not_multiple_of_8():
    """the V pass reads 16-byte chunks up to round_up(total, 8) of rows of length smax: smax = 13 is refused by the three unfused
    entry points as by every other one (the caches here hold 16 positions: nothing could be read outside them either way)"""
    L = _lib()
    batch, nh = 1, 2
    q = torch.zeros((batch, nh, HD), dtype=BF, device=DEV)
    k = torch.zeros((batch, nh, 16, HD), dtype=BF, device=DEV)
    vt = torch.zeros((batch, nh, HD, 16), dtype=BF, device=DEV)
    out = torch.zeros((batch, nh * HD), dtype=BF, device=DEV)
    pos = torch.tensor([11], dtype=torch.int32, device=DEV)
    slopes = R.alibi_slopes(nh).to(DEV)
    p = lambda t: t.data_ptr()
    assert L.llark_attn_decode_bf16(p(q), p(k), p(vt), None, None, None, batch, nh, HD, 12, 13, p(out), None, _stream()) == ERR_INVALID
    assert L.llark_attn_decode_bf16_alibi(p(q), p(k), p(vt), None, None, None, batch, nh, HD, 12, 13, p(out), None, p(slopes), _stream()) == ERR_INVALID
    assert L.llark_attn_decode_bf16_dpos(p(q), p(k), p(vt), None, None, None, batch, nh, HD, p(pos), 13, p(out), None, _stream()) == ERR_INVALID
    _sync()


# =====================================================================================================================
# 3. RoPE + head split + cache write: rope_split_kernel
# =====================================================================================================================
ROPE_SHAPES = [(1, 1, 1, 0), (2, 3, 65, 0), (1, 2, 64, 37), (2, 2, 5, 200), (1, 2, 130, 8)]
ROPE_DPOS = [(1, 1, 1, 0), (2, 3, 1, 200)]


def _rope_case(batch, nh, s, pos0, with_lo, dpos):
    ops = _ops()
    H, N = nh * HD, batch * nh
    smax = R.round_up(pos0 + s + 3, 8) + 8
    g = _gen(batch, nh, s, pos0, 5)
    qkv = torch.randn(batch * s, 3 * H, generator=g) * 2
    cos, sin = R.rope_tables(smax)
    d_qkv, d_cos, d_sin = qkv.to(DEV), cos.to(DEV), sin.to(DEV)
    nplanes = 2 if with_lo else 1
    q_out = [_Out(N * s * HD) for _ in range(nplanes)]
    k_host = [_bf_sentinel((batch, nh, smax, HD)) for _ in range(nplanes)]
    v_host = [_bf_sentinel((batch, nh, HD, smax)) for _ in range(nplanes)]
    k_dev, v_dev = [t.to(DEV) for t in k_host], [t.to(DEV) for t in v_host]
    qv = [o.view.view(batch, nh, s, HD) for o in q_out]
    lo = (lambda ps: ps[1]) if with_lo else (lambda ps: None)
    if dpos:
        d_pos = torch.tensor([pos0], dtype=torch.int32, device=DEV)
        ops.rope_split_heads_dpos(d_qkv, batch, nh, HD, d_pos, d_cos, d_sin, qv[0], k_dev[0], v_dev[0], lo(qv), lo(k_dev), lo(v_dev))
    else:
        ops.rope_split_heads(d_qkv, batch, s, nh, HD, pos0, d_cos, d_sin, qv[0], k_dev[0], v_dev[0], lo(qv), lo(k_dev), lo(v_dev))
    _sync()
    _same("qkv", d_qkv, qkv), _same("cos", d_cos, cos), _same("sin", d_sin, sin)
    x = qkv.view(batch, s, 3, nh, HD).permute(2, 0, 3, 1, 4)                     # [3][batch][nh][s][128]
    c, sn = cos[pos0:pos0 + s], sin[pos0:pos0 + s]
    kw = torch.zeros((batch, nh, smax, HD), dtype=torch.bool)
    kw[:, :, pos0:pos0 + s] = True
    vw = torch.zeros((batch, nh, HD, smax), dtype=torch.bool)
    vw[..., pos0:pos0 + s] = True
    q_got = [o.result("q").view(batch, nh, s, HD) for o in q_out]
    for i in range(nplanes):
        _assert_untouched(f"k cache plane {i}", k_dev[i], k_host[i], kw)
        _assert_untouched(f"v^T cache plane {i}", v_dev[i], v_host[i], vw)
    k_got = [t.cpu()[:, :, pos0:pos0 + s] for t in k_dev]
    v_got = [t.cpu()[..., pos0:pos0 + s] for t in v_dev]
    tag = f"rope {batch}x{nh}x{s}@{pos0}{' lo' if with_lo else ''}{' dpos' if dpos else ''}"
    for nm, xi, got in (("q", x[0], q_got), ("k", x[1], k_got)):
        ref = R.rope(xi, c, sn)
        fp32 = 4.0 * EPS24 * R.rope_bound(xi, c, sn).numpy()
        _check_frac(f"{tag} {nm} hi", got[0].double(), ref, _bf16_ulp(ref) + fp32, 0.0)
        if with_lo:
            _check_frac(f"{tag} {nm} hi+lo", got[0].double() + got[1].double(), ref, 2.0 ** -16 * ref.abs().numpy() + fp32, 0.0)
        want = R.planes(R.rope(xi, c, sn, torch.float32))          # the kernel's own float32 expression: bit-equal planes
        for i in range(nplanes):
            assert torch.equal(_bits(got[i]), _bits(want[i])), f"{tag} {nm} plane {i} differs from torch's float32 rotation"
    vwant = R.planes(x[2].transpose(2, 3).contiguous())
    for i in range(nplanes):
        assert torch.equal(_bits(v_got[i]), _bits(vwant[i])), f"{tag} v^T plane {i}"


@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("batch,nh,s,pos0", ROPE_SHAPES)
def test_rope_split_heads(batch, nh, s, pos0, with_lo):
    """the rotation's sign or partner, pos0 ignored in the table row or the cache row, a token of the ragged last 64-token block
    written twice or not at all, the lo plane taken of the wrong value, V transposed into the wrong column"""
    _rope_case(batch, nh, s, pos0, with_lo, False)


@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("batch,nh,s,pos0", ROPE_DPOS)
def test_rope_split_heads_dpos(batch, nh, s, pos0, with_lo):
    """the position read from device memory: used for the table row AND the cache row / column"""
    _rope_case(batch, nh, s, pos0, with_lo, True)


# =====================================================================================================================
# 4. RMSNorm: rmsnorm_kernel<NV>, NV = 1 | 4 | 16 | 32
# =====================================================================================================================
RMS_WIDTHS = [4, 256, 260, 1024, 1028, 4096, 4100, 8192]          # both sides of every NV switch (width / 4 <= 64, 256, 1024, 2048)


@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("rows", [1, 4, 5])
@pytest.mark.parametrize("width", RMS_WIDTHS)
def test_rmsnorm(width, rows, with_lo):
    """a row handed to the wrong wave of its block of four, the tail float4 of a width that does not fill the last 64-lane pass, eps
    outside the square root, the mean over ldx or over the padded width, a row stride confused between input and output"""
    L = _lib()
    ldx, ldo, eps = width + 4, width + 8, 1e-5
    g = _gen(width, rows, 3)
    x = torch.randn(rows, width, generator=g) * 2
    w = 1 + 0.2 * torch.randn(width, generator=g)
    special = [lambda r: r * 1e-3, lambda r: r * 1e3, lambda r: r * 0.0, lambda r: torch.where(torch.arange(width) == width // 3, r, torch.zeros(()))]
    for i in range(min(rows, 4) if rows > 1 else 0):
        x[i] = special[i](x[i])
    xbuf = torch.full((rows, ldx), float("nan"))
    xbuf[:, :width] = x
    d_x, d_w = xbuf.to(DEV), w.to(DEV)
    outs = [_Out(rows * ldo) for _ in range(2 if with_lo else 1)]
    written = torch.zeros(PAD + rows * ldo + PAD, dtype=torch.bool)
    written[PAD:PAD + rows * ldo].view(rows, ldo)[:, :width] = True
    rc = L.llark_rmsnorm_bf16(d_x.data_ptr(), ldx, rows, width, d_w.data_ptr(), float(np.float32(eps)), outs[0].view.data_ptr(),
                              outs[1].view.data_ptr() if with_lo else None, ldo, _stream())
    assert rc == 0
    _sync()
    _same("x", d_x, xbuf), _same("w", d_w, w)
    got = [o.result("rmsnorm out", written).view(rows, ldo)[:, :width].double() for o in outs]
    eps32 = float(np.float32(eps))
    ref, rstd = R.rmsnorm(x, w, eps32)
    t32, _ = R.rmsnorm(x, w, eps32, torch.float32)
    atol32, r = _tol("rmsnorm", t32, ref, w.double().abs() * x.double().abs() * rstd)
    tag = f"rmsnorm {rows}x{width}"
    _check_frac(f"{tag} hi", got[0], ref, _bf16_ulp(ref) + atol32, r)
    if with_lo:
        _check_frac(f"{tag} hi+lo", got[0] + got[1], ref, 2.0 ** -16 * ref.abs().numpy() + atol32, r)


def test_rmsnorm_width_8196_unsupported():
    L = _lib()
    x = torch.zeros((1, 8196), device=DEV)
    w = torch.ones(8196, device=DEV)
    out = _Out(8196)
    assert L.llark_rmsnorm_bf16(x.data_ptr(), 8196, 1, 8196, w.data_ptr(), 1e-5, out.view.data_ptr(), None, 8196, _stream()) == ERR_UNSUPPORTED
    _sync()
    out.result("rmsnorm 8196", torch.zeros_like(out.mask))


# =====================================================================================================================
# 5. embedding gather: embed_gather_kernel<T>
# =====================================================================================================================
@pytest.mark.parametrize("dtype,code", [(torch.bfloat16, 1), (torch.float16, 0), (torch.float32, 2)], ids=["bf16", "fp16", "fp32"])
def test_embed_gather(dtype, code):
    """a row index off by one, the table read as another type, columns past one 256-thread pass dropped (width 250 is no multiple of the
    block), ids outside [0, vocab) reading outside the table: the kernel clamps them to the first / last row"""
    L = _lib()
    vocab, width, ldo = 37, 250, 256
    g = _gen(vocab, width, code)
    table = torch.randn(vocab, width, generator=g).to(dtype)
    ids = torch.tensor([5, -3, vocab + 2, 0, vocab - 1, 17, 5], dtype=torch.int64)
    rows = ids.numel()
    d_table, d_ids = table.to(DEV), ids.to(DEV)
    n = rows * ldo
    host, m = _out_slab(n, torch.float32)                          # odd offset: the kernel stores single floats
    dev = host.to(DEV)
    written = torch.zeros_like(m)
    written[3:3 + n].view(rows, ldo)[:, :width] = True
    assert L.llark_embed_gather(d_ids.data_ptr(), rows, d_table.data_ptr(), code, vocab, width, dev[3:].data_ptr(), ldo, _stream()) == 0
    _sync()
    _same("table", d_table, table), _same("ids", d_ids, ids)
    _assert_untouched("embed_gather", dev, host, written)
    got = dev.cpu()[3:3 + n].view(rows, ldo)[:, :width]
    want = R.embed(ids, table)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(got[1], table[0].float()) and torch.equal(got[2], table[vocab - 1].float())      # the clamp
