"""The flash attention backward of csrc/attn_bwd.hip -- attn_bwd_rowdot_kernel, attn_bwd_dkv_kernel, attn_bwd_dq_kernel behind
llark_attn_backward_bf16 and llark_attn_backward_bf16_fused -- element by element against the float64 contract reference of
tests/attn_bwd_ref.py, at its tile and grid edges.

Isolated (``test_attn_backward``): o (bf16) and lse (fp32) come from the float64 forward, so the backward is judged as the function of
its operands the header promises.  dq, dk, dv and dsum are each compared with the reference under the per-element bounds of
attn_bwd_ref (format terms u = 2^-8 for the one rounding of P and of dS, plus c 2^-24 times the fp32 error sums, c from torch's own
float32 CPU run of the same function).  The keys are PLANTED (``k_j += 0.35 q_i``) on the diagonal at every wave and tile edge, at the
first key of every 64-key tile seen from a little below the diagonal, at the last key, and on the first masked key of a few queries;
K-cache rows >= s hold the largest finite bf16, not zeros.  Every output lies in a NaN slab at a 16-byte-aligned offset and the slab
is asserted bit-unchanged around it; every output is finite; q, the K cache with its garbage rows, v, dO, o and lse are bit-unchanged;
a second launch is bit-equal to the first (no atomics, a fixed order).  tests/test_attn_bwd_ref_cpu.py shows on the CPU that these
bounds accept the kernel's arithmetic and reject a dropped or extra (query, key) pair, a wrong D, a lost factor and a tile taken twice.

Chained (``test_attn_backward_chained``): o and lse from llark_attn_prefill_bf16_lse as in the engines, the reference fed the same o and
lse, the bounds unchanged.  Fused (``test_attn_backward_fused``): llark_attn_backward_bf16_fused with a dO pitch of nh 128 + 64 whose
padding columns hold NaN, at pos0 0 and 24, bit-equal in dqkv and dsum to llark_split_heads16 + llark_attn_backward_bf16 +
llark_rope_merge_bwd (float64-tested in test_train_kernels_gpu.py), sentinels around dqkv untouched; it needs no float64 reference
and runs on every case without ALiBi.

Case ids are built from attn_bwd_ref.backward_rule, the restatement of grid_of / block_to_pair: paired or single tiles per workgroup,
the tile count nt, the workgroups per head np, whether the middle tile stands alone, XCD or linear numbering.  The float64 reference
of the four largest cases (8 x 32 x 256, 8 x 32 x 450, 171 x 12 x 100, 171 x 6 x 130: more than 8e6 scores) is evaluated by the same
function in float64 on the device; torch's float32 run that sets ``c`` is on the CPU for every case.

Measured on the MI355X, worst over the cases (kernel error as a fraction of the tolerance | torch float32 ``r`` in units of 2^-24 times
the fp32 bound; ``-s`` prints each case's own "[ratio] ..." lines):

    output      isolated: kernel / tolerance | r        chained: kernel / tolerance | r
    dq          0.94 | 0.89                             0.80 | 0.55
    dk          0.93 | 0.71                             0.87 | 0.55
    dv          0.98 | 1.50                             0.97 | 1.08
    dsum        0.06 | 1.39                             0.05 | 0.97

``c`` was 16 in every case (r < 4).  The kernel's fractions equal those of attn_bwd_ref.emulate on the cases the CPU file runs to the
printed digits (0.712 | 0.747 | 0.900 at 2 x 4 x 200 with ALiBi, 0.886 | 0.909 | 0.952 at 8 x 32 x 130 with ALiBi): what the kernel adds
to the two bf16 roundings is not visible.  dv sits near 1 by construction where one probability dominates a column: round to nearest
errs by up to half an ulp, which is 2^-8 P just above a power of two -- the whole of ``u``.  At S = 1 dq and dk came out exactly 0.
The whole file: 29 cases in 25 s on the MI355X; the slowest, 171 x 12 x 100, takes 5 s, of which the launches are milliseconds and the
rest is the shared tolerance arithmetic over 3 x 26 M float64 elements on the host.
"""
import functools

import pytest
import torch

import attn_bwd_ref as R
from kernel_util import assert_untouched as _assert_untouched, bits as _bits, out_slab as _out_slab
from llama_kernel_ref import from_rows, rope_tables, to_rows, vt_cache

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = R.HD
BF, F32 = torch.bfloat16, torch.float32
PAD = {F32: 4, BF: 8}                             # elements in front of an output inside its slab: 16 bytes


def _ops():
    from llark_amd import ops
    return ops


class _Out:
    """an output of ``n`` elements inside a sentinel slab on the device, 16 bytes in"""

    def __init__(self, n, dtype=F32):
        self.n, self.pad = n, PAD[dtype]
        self.host, self.mask = _out_slab(n, dtype, front=self.pad, back=self.pad)
        self.dev = self.host.to(DEV)
        self.view = self.dev[self.pad:self.pad + n]
        assert self.view.data_ptr() % 16 == 0

    def result(self, name):
        """the output on the host, after asserting that nothing around it was touched"""
        _assert_untouched(name, self.dev, self.host, self.mask)
        return self.dev.cpu()[self.pad:self.pad + self.n]


def _same(name, dev_t, host_t):
    assert torch.equal(_bits(dev_t), _bits(host_t)), f"{name}: an input was modified"


@functools.lru_cache(maxsize=1)
def _data(case):
    """the operands of a case on the host and on the device: q, v, dO [N][S][128], the K cache [batch][nh][smax][128] with garbage rows"""
    batch, nh, s, smax, alibi = case
    o = R.operands(batch, nh, s)
    host = {"q": o["q"], "kc": R.k_cache(o["k"], batch, nh, smax), "v": o["v"], "dO": o["dO"]}
    if alibi:
        host["slopes"] = R.alibi_slopes(nh)
    return o, host, {n: t.to(DEV) for n, t in host.items()}


@functools.lru_cache(maxsize=1)
def _reference(case):
    """o, lse of the float64 forward and the contract reference on them"""
    o = _data(case)[0]
    dev = DEV if R.on_device(case) else None
    slopes = R.slopes_of(case)
    out, lse = R.forward(o, slopes, device=dev)
    R.planted_p(case, o, slopes)
    return out, lse, R.reference(o["q"], o["k"], o["v"], o["dO"], out, lse, slopes, device=dev)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_data():
    yield
    _data.cache_clear()
    _reference.cache_clear()


def _launch(case, dev, o_rows, lse):
    """one launch of llark_attn_backward_bf16 into fresh slabs"""
    batch, nh, s, _, _ = case
    N = batch * nh
    outs = {n: _Out(N * s * HD) for n in ("dq", "dk", "dv")}
    outs["dsum"] = _Out(N * s)
    v3 = lambda n: outs[n].view.view(N, s, HD)
    _ops().attn_backward(dev["q"], dev["kc"], dev["v"], dev["dO"], o_rows, lse, outs["dsum"].view.view(N, s), batch, s, nh, HD,
                         v3("dq"), v3("dk"), v3("dv"), alibi_slopes=dev.get("slopes"))
    torch.cuda.synchronize()
    return outs


def _backward(case, dev, o_rows, lse, twice=False):
    """the outputs on the host as [N][S][128] / [N][S]: nothing around them written, all finite; ``twice``: a second launch into other
    slabs is bit-equal (compared on the device, the whole slabs)"""
    batch, nh, s, _, _ = case
    N = batch * nh
    outs = _launch(case, dev, o_rows, lse)
    if twice:
        for n, again in _launch(case, dev, o_rows, lse).items():
            assert torch.equal(again.dev.view(torch.int32), outs[n].dev.view(torch.int32)), f"{n}: a second launch differs"
    got = {n: outs[n].result(n).view((N, s, HD) if n != "dsum" else (N, s)) for n in outs}
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{n}: non-finite values"
    return got


def _inputs_unchanged(dev, host, extra):
    for n, t in host.items():
        _same(n, dev[n], t)
    for n, (d, h) in extra.items():
        _same(n, d, h)


@pytest.mark.parametrize("case", list(R.CASES), ids=R.case_id)
def test_attn_backward(case):
    """a (query, key) pair lost, doubled or shown at a tile, wave or grid edge; a row >= s read from the K cache; D, lse or an operand
    row of the wrong query; a tile handed to the wrong workgroup or taken twice (paired grids, both numberings); a lost factor scale"""
    batch, nh, s, smax, _ = case
    rule = R.backward_rule(batch, nh, s)
    assert (rule.paired, rule.xcd, rule.np, rule.middle) == R.CASES[case]
    _, host, dev = _data(case)
    out, lse, ref = _reference(case)
    o_rows_h = to_rows(out, batch, nh).contiguous()
    o_rows, lse_d = o_rows_h.to(DEV), lse.to(DEV)
    got = _backward(case, dev, o_rows, lse_d, twice=True)
    _inputs_unchanged(dev, host, {"o": (o_rows, o_rows_h), "lse": (lse_d, lse)})
    R.check(R.case_id(case), got, ref)


@pytest.mark.parametrize("case", R.CHAINED, ids=R.case_id)
def test_attn_backward_chained(case):
    """the backward on what the training forward leaves: o and lse of llark_attn_prefill_bf16_lse, the reference fed the same two"""
    batch, nh, s, smax, _ = case
    N = batch * nh
    o, host, dev = _data(case)
    vt = vt_cache(o["v"], batch, nh, smax).to(DEV)
    o_rows = torch.empty((batch * s, nh * HD), dtype=BF, device=DEV)
    lse = torch.empty((N, s), dtype=F32, device=DEV)
    _ops().attn_prefill_lse(dev["q"].view(batch, nh, s, HD), dev["kc"], vt, batch, s, nh, HD, o_rows, lse, alibi_slopes=dev.get("slopes"))
    torch.cuda.synchronize()
    o_rows_h, lse_h = o_rows.cpu(), lse.cpu()
    got = _backward(case, dev, o_rows, lse)
    _inputs_unchanged(dev, host, {"o": (o_rows, o_rows_h), "lse": (lse, lse_h)})
    ref = R.reference(o["q"], o["k"], o["v"], o["dO"], from_rows(o_rows_h, batch, nh), lse_h, R.slopes_of(case),
                      device=DEV if R.on_device(case) else None)
    R.check("chained " + R.case_id(case), got, ref)


@pytest.mark.parametrize("case", [c for c in R.CASES if not c[4]], ids=R.case_id)
def test_attn_backward_fused(case):
    """dO read token-major at a wider pitch (a head's columns, not the padding), d(q | k | v) written through the RoPE epilogue at the
    rows of pos0: bit-equal to the separate passes, nothing written around dqkv"""
    ops = _ops()
    batch, nh, s, smax, _ = case
    N, H = batch * nh, nh * HD
    o, host, dev = _data(case)
    vt = vt_cache(o["v"], batch, nh, smax).to(DEV)
    o_rows = torch.empty((batch * s, H), dtype=BF, device=DEV)
    lse = torch.empty((N, s), dtype=F32, device=DEV)
    ops.attn_prefill_lse(dev["q"].view(batch, nh, s, HD), dev["kc"], vt, batch, s, nh, HD, o_rows, lse)
    dbuf_h = torch.full((batch * s, H + 64), float("nan"), dtype=BF)
    dbuf_h[:, :H] = to_rows(o["dO"], batch, nh)
    dbuf = dbuf_h.to(DEV)
    datt = dbuf[:, :H]
    dO = torch.empty((N, s, HD), dtype=BF, device=DEV)
    ops.split_heads16(datt.contiguous(), batch, s, nh, HD, dO)
    assert torch.equal(_bits(dO), _bits(o["dO"]))
    dq, dk, dv = (torch.empty((N, s, HD), dtype=F32, device=DEV) for _ in range(3))
    dsum = torch.empty((N, s), dtype=F32, device=DEV)
    ops.attn_backward(dev["q"], dev["kc"], dev["v"], dO, o_rows, lse, dsum, batch, s, nh, HD, dq, dk, dv)
    cos_t, sin_t = (t.to(DEV) for t in rope_tables(24 + s))
    for pos0 in (0, 24):
        want = torch.empty((batch * s, 3 * H), dtype=BF, device=DEV)
        ops.rope_merge_bwd(dq, dk, dv, cos_t, sin_t, batch, s, nh, HD, pos0, want)
        out = _Out(batch * s * 3 * H, BF)
        dsum2 = _Out(N * s)
        ops.attn_backward_fused(dev["q"], dev["kc"], dev["v"], datt, o_rows, lse, dsum2.view.view(N, s), batch, s, nh, HD, cos_t, sin_t, pos0,
                                out.view.view(batch * s, 3 * H))
        torch.cuda.synchronize()
        got = out.result(f"dqkv pos0={pos0}")
        assert bool(torch.isfinite(got.float()).all()), "dqkv: non-finite values (a padding column of dO was read)"
        assert torch.equal(_bits(got), _bits(want).reshape(-1)), f"dqkv pos0={pos0}: {int((_bits(got) != _bits(want).reshape(-1)).sum())} elements differ"
        assert torch.equal(_bits(dsum2.result("dsum")), _bits(dsum).reshape(-1)), f"dsum pos0={pos0}"
        assert float(want.float().abs().max()) > 0
    _inputs_unchanged(dev, host, {"dO token-major": (dbuf, dbuf_h)})
