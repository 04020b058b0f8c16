"""The checker of tests/test_llama_kernels_gpu.py has teeth, shown without running a kernel: the float64 references and bounds of
tests/llama_kernel_ref.py reject CPU stand-ins for wrong kernels -- a planted key dropped, the first masked key admitted, the key at
``total`` admitted, the running maximum taken over a quarter of the keys -- and accept a float32 / bf16-flow emulation of the correct
arithmetic, through the same ``check_out`` / ``check_lse`` calls the GPU tests make.  Shapes: prefill (1, 2, 130, 37), decode at
total = 129.  The launcher-rule helper is checked against every prefill shape of the GPU file, so that a shape which stops reaching
its branch is noticed here.

One combination cannot be rejected and is asserted ACCEPTED instead: the quarter maximum with ONE bf16 probability plane (the
``lse`` bound).  exp(s - m) / sum exp(s - m) does not depend on m, and a bf16 rounding is a relative error of 2^-9 at any magnitude,
so that stand-in is a correct softmax in that number format (here it reaches 0.85 of the bound, the emulation 0.69).  Against the
bounds whose probabilities carry 16 bits (decode, bf16 and split prefill) the single bf16 plane is what fails it.
"""
import pytest
import torch

import llama_kernel_ref as R

PREFILL = (1, 2, 130, 37)
DECODE_TOTAL = 129
KINDS = ["bf16", "split", "lse", "decode", "decode_split"]


def test_launcher_rule_reaches_every_branch():
    for (batch, nh, s, past), (nq, paired, xcd, nt) in R.PREFILL_SHAPES.items():
        r = R.prefill_rule(batch, nh, s, False)
        assert (r.nq, r.paired, r.xcd, r.nt) == (nq, paired, xcd, nt), (batch, nh, s, past, vars(r))
        assert R.prefill_rule(batch, nh, s, True).nq == 1
    for (batch, nh, s, past), (paired, nt) in R.PREFILL_SPLIT_LARGE.items():
        r = R.prefill_rule(batch, nh, s, True)
        assert (r.paired, r.nt) == (paired, nt), (batch, nh, s, vars(r))
    # every branch is there: both NQ, paired with an even and an odd block count for both, both numberings unpaired
    seen = {(nq, paired, nt % 2 if paired else None) for nq, paired, _, nt in R.PREFILL_SHAPES.values()}
    assert seen >= {(1, False, None), (2, False, None), (1, True, 0), (1, True, 1), (2, True, 0), (2, True, 1)}
    assert {(nq, xcd) for nq, paired, xcd, _ in R.PREFILL_SHAPES.values() if not paired} == {(1, False), (1, True), (2, False), (2, True)}
    assert {p for p, _ in R.PREFILL_SPLIT_LARGE.values()} == {True, False}
    assert [R.decode_waves(b, h) for b, h in [(1, 2), (3, 32), (8, 32), (16, 32)]] == [16, 16, 4, 4]
    assert "<0,2,1,0>-paired-nt3-xcd" in R.prefill_case_id((16, 32, 300, 0), "bf16", False)


def test_plants_cover_the_edges():
    for (batch, nh, s, past), (nq, *_rest) in R.PREFILL_SHAPES.items():
        total = past + s
        vis, masked = R.prefill_plants(s, past, nq)
        assert all(0 <= i < s and 0 <= j <= past + i for i, j in vis) and all(j == past + i + 1 < total for i, j in masked)
        keys = {j for _, j in vis}
        assert {past, total - 1} <= keys and (past > 0) <= (0 in keys)
        for j in (63, 64, 64 * (total // 64)):
            assert j in keys or not (0 <= j < total), (s, past, j)
    for total in (1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257, 371, 513):
        keys = R.decode_plants(total)
        assert {0, total - 1} <= set(keys) and all(0 <= j < total for j in keys)
        for edge in (128, 256):                                                   # either side of each round boundary
            assert {edge - 1, edge} & set(range(total)) <= set(keys)


def _operands(kind):
    split = kind in ("split", "decode_split")
    if kind.startswith("decode"):
        total, N = DECODE_TOTAL, 2
        g = R.gen(total, 5)
        q = torch.randn(N, 1, R.HD, generator=g) * 1.5
        k = torch.randn(N, total, R.HD, generator=g) * 1.5
        v = torch.randn(N, total, R.HD, generator=g)
        keys = R.decode_plants(total)
        for j in keys:
            k[:, j] += R.PLANT * q[:, 0]
        cut = R.planes if split else (lambda x: (x.bfloat16(), None))
        o = {"q": cut(q), "k": cut(k), "v": cut(v)}
        return o, total - 1, (0, keys[len(keys) // 2])
    batch, nh, s, past = PREFILL
    vis, _ = R.prefill_plants(s, past, 1)
    return R.prefill_operands(batch, nh, s, past, split), past, next(p for p in vis if p[0] == 16)


@pytest.fixture(scope="module", params=[(k, a) for k in KINDS for a in (False, True)], ids=lambda p: f"{p[0]}{'_alibi' if p[1] else ''}")
def case(request):
    kind, alibi = request.param
    o, past, drop = _operands(kind)
    q, k, v = (R.value(*o[n]) for n in "qkv")
    slopes = R.alibi_slopes(2).double() if alibi else None
    return dict(kind=kind, q=q, k=k, v=v, past=past, slopes=slopes, drop=drop, ref=R.reference(q, k, v, past, slopes))


def _causal(c):
    S, T = c["q"].shape[1], c["k"].shape[1]
    return torch.arange(T)[None, :] <= c["past"] + torch.arange(S)[:, None]


def _with_key_at_total(c):
    """operands with the cache position ``total`` appended as the GPU tests leave it: the largest finite bf16 in every plane"""
    N = c["q"].shape[0]
    row = R.garbage((N, 1, R.HD)).double() * (2.0 if c["kind"] in R.TWO_PLANES else 1.0)
    vis = torch.cat((_causal(c), torch.zeros((c["q"].shape[1], 1), dtype=torch.bool)), dim=1)
    return torch.cat((c["k"], row), dim=1), torch.cat((c["v"], row), dim=1), vis


def _rejected(name, c, got):
    with pytest.raises(AssertionError):
        R.check_out(name, c["kind"], got, c["ref"])


def test_correct_emulation_is_accepted(case):
    c = case
    got, lse = R.emulate(c["kind"], c["q"], c["k"], c["v"], c["past"], c["slopes"])
    R.check_out(f"{c['kind']} emulation", c["kind"], got, c["ref"])
    R.check_lse(f"{c['kind']} emulation lse", lse.double(), c["ref"])


def test_dropped_planted_key_is_rejected(case):
    c = case
    vis = _causal(c)
    i, j = c["drop"]
    assert vis[i, j]
    vis[i, j] = False
    got, lse = R.emulate(c["kind"], c["q"], c["k"], c["v"], c["past"], c["slopes"], visible=vis)
    _rejected("planted key dropped", c, got)
    with pytest.raises(AssertionError):
        R.check_lse("planted key dropped: lse", lse.double(), c["ref"])


def test_first_masked_key_admitted_is_rejected(case):
    c = case
    if c["kind"].startswith("decode"):                       # one query: its first masked key is the key at `total`
        k, v, vis = _with_key_at_total(c)
        vis[0, -1] = True
    else:
        k, v, vis = c["k"], c["v"], _causal(c)
        i = torch.arange(vis.shape[0] - 1)
        vis[i, c["past"] + i + 1] = True                     # the mask one key late
    total = c["past"] + c["q"].shape[1]
    got, _ = R.emulate(c["kind"], c["q"], k, v, c["past"], c["slopes"], visible=vis, total=total)
    _rejected("first masked key admitted", c, got)


def test_key_at_total_admitted_is_rejected(case):
    c = case
    k, v, vis = _with_key_at_total(c)
    vis[-1, -1] = True                                       # the last query also sees cache position `total`
    total = c["past"] + c["q"].shape[1]
    got, _ = R.emulate(c["kind"], c["q"], k, v, c["past"], c["slopes"], visible=vis, total=total)
    _rejected("key at total admitted", c, got)


def test_quarter_maximum_is_rejected(case):
    """the defect recorded in csrc/llama.hip at the all-reduce of the row maximum: the maximum over a quarter of the keys,
    probabilities renormalised against it and rounded to bf16"""
    c = case
    got, _ = R.emulate(c["kind"], c["q"], c["k"], c["v"], c["past"], c["slopes"], quarter_max=True)
    if c["kind"] == "lse":                                   # see the module docstring: a correct softmax in this format
        assert R.check_out("quarter maximum, one p plane", "lse", got, c["ref"]) >= 0.0
    else:
        _rejected("quarter maximum", c, got)
