"""The checker of tests/test_attn_bwd_kernels_gpu.py has teeth, shown without running a kernel.

* With unrounded o and lse the contract reference of tests/attn_bwd_ref.py IS the derivative: it equals float64 autograd of
  softmax(mask(scale q k^T + bias)) v to 1e-10 relative, with and without ALiBi.
* ``emulate`` -- the kernel's two bf16 roundings, float32 exponent, exact accumulation -- stays inside the bounds on every GPU case
  whose reference runs on the CPU.  Left out (their float64 reference runs on the device in the GPU file): 8 x 32 x 256, 8 x 32 x 450,
  171 x 12 x 100 and 171 x 6 x 130.
* The same ``check`` call rejects stand-ins for wrong kernels (``-s`` prints by how much, as "[ratio] ..." lines): a visible key dropped
  at a tile edge, the first masked key shown, a phantom query row >= S, a phantom key >= S, D from the neighbouring row, dK without its
  factor scale, the middle tile of an odd paired grid accumulated twice, the ALiBi bias referenced to key - query.
* ``backward_rule`` gives the (paired, xcd, np, middle) each GPU case is there for.

Phantom rows.  The kernels stage the ragged tile with ZERO rows past S (queries in the dK / dV kernel: q = dO = 0, lse = D = 0, so
P = 1; keys in the dQ kernel: k = v = 0).  Such a row contributes nothing even when the mask lets it through -- dV += 1 * 0,
dS = 1 * (0 - 0), dQ += dS * 0 -- which ``test_zero_filled_phantom_rows_are_harmless`` asserts bit for bit: no test can reject that,
and the zero fill is itself a guard.  What is rejected is the phantom row carrying the CLAMPED operand row S - 1, which is how these
kernels read every other operand row past S (the fragment loads of both kernels).
"""
import functools

import pytest
import torch

import attn_bwd_ref as R

CPU_CASES = [c for c in R.CASES if not R.on_device(c)]
BASE = (1, 2, 130, 256, False)           # three tiles, the last ragged
ODD_PAIRED = (8, 32, 130, 136, False)
ALIBI = (2, 4, 200, 256, True)


@functools.lru_cache(maxsize=2)
def _case(case):
    batch, nh, s, _, _ = case
    ops = R.operands(batch, nh, s)
    slopes = R.slopes_of(case)
    o, lse = R.forward(ops, slopes)
    R.planted_p(case, ops, slopes)
    ref = R.reference(ops["q"], ops["k"], ops["v"], ops["dO"], o, lse, slopes)
    return SimpleCase(ops, slopes, o, lse, ref)


class SimpleCase:
    def __init__(self, ops, slopes, o, lse, ref):
        self.ops, self.slopes, self.o, self.lse, self.ref = ops, slopes, o, lse, ref
        self.args = (ops["q"], ops["k"], ops["v"], ops["dO"], o, lse, slopes)


def test_backward_rule_reaches_every_path():
    for case, want in R.CASES.items():
        r = R.backward_rule(*case[:3])
        assert (r.paired, r.xcd, r.np, r.middle) == want, (case, vars(r))
        assert case[2] <= case[3]
    rules = [R.backward_rule(*c[:3]) for c in R.CASES]
    assert {(r.paired, r.xcd) for r in rules} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(r.np, r.middle, r.xcd) for r in rules if r.paired} >= {(1, False, True), (2, True, True), (2, False, True), (4, False, True),
                                                                   (1, False, False), (2, True, False)}
    assert {r.workgroups for r in rules if r.paired} >= {512, 1024}
    assert R.case_id((8, 32, 130, 136, True)) == "alibi-8x32x130m136-paired-nt3-np2-middle-xcd"
    assert all(c in R.CASES for c in R.CHAINED)


def test_plants_cover_the_edges():
    for case in R.CASES:
        s = case[2]
        vis, masked = R.plants(s)
        assert all(0 <= j <= i < s for i, j in vis) and all(j == i + 1 < s for i, j in masked)
        assert {(i, i) for i in (0, 15, 16, 31, 32, 47, 48, 63, 64, s - 1) if i < s} <= set(vis)
        below = {j for i, j in vis if i == min(s - 1, j + 3)}          # seen from a little below the diagonal
        assert {j for j in {0, 63, 64, s - 1} | set(range(0, s, 64)) if j < s} <= below


@pytest.mark.parametrize("alibi", [False, True], ids=["plain", "alibi"])
def test_contract_reference_is_the_derivative(alibi):
    N, S = 3, 70
    g = R.gen(N, S, 7)
    q, k, v = (torch.randn(N, S, R.HD, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3))
    dO = torch.randn(N, S, R.HD, generator=g, dtype=torch.float64)
    slopes = R.alibi_slopes(N).double() if alibi else None
    s = torch.matmul(q, k.transpose(1, 2)) * R.SCALE
    if alibi:
        s = s + slopes[:, None, None] * (torch.arange(S) - (S - 1)).double()[None, None, :]
    s = s.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
    o = torch.matmul(torch.softmax(s, -1), v)
    o.backward(dO)
    lse = torch.logsumexp(s, -1)
    got = R.backward(q.detach(), k.detach(), v.detach(), dO, o.detach(), lse.detach(), slopes, bounds=False)
    for name, want in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        rel = float((getattr(got, name) - want).abs().max() / want.abs().max())
        print(f"[autograd] {name}: {rel:.2e}")
        assert rel <= 1e-10, (name, rel)
    assert torch.equal(got.dsum, (dO * o.detach()).sum(-1))


@pytest.mark.parametrize("case", CPU_CASES, ids=R.case_id)
def test_correct_emulation_is_accepted(case):
    c = _case(case)
    R.check(f"emulation {R.case_id(case)}", R.emulate(*c.args), c.ref)


def _rejected(tag, c, got):
    """beyond the tolerance for at least one of dq, dk, dv (outputs with appended phantom rows are cut back to S); returns which"""
    S = c.o.shape[1]
    got = {n: t[:, :S] for n, t in got.items()}
    bad = []
    for name in ("dq", "dk", "dv"):
        try:
            R.check(tag, got, c.ref, only=(name,))
        except AssertionError:
            bad.append(name)
    print(f"[rejected] {tag}: {bad}")
    assert bad, f"{tag}: accepted"
    return bad


def test_dropped_key_at_a_tile_edge_is_rejected():
    c = _case(BASE)
    vis = R._causal(130, 130)
    assert vis[67, 64] and (67, 64) in R.plants(130)[0]
    vis[67, 64] = False                                     # the first key of the second tile, for one query
    _rejected("key 64 dropped for query 67", c, R.emulate(*c.args, visible=vis))


def test_first_masked_key_shown_is_rejected():
    c = _case(BASE)
    vis = R._causal(130, 130)
    vis[63, 64] = True                                      # across the tile edge
    _rejected("masked key 64 shown to query 63", c, R.emulate(*c.args, visible=vis))
    vis = R._causal(130, 130)
    i = torch.arange(129)
    vis[i, i + 1] = True                                    # the whole mask one key late
    _rejected("mask one key late", c, R.emulate(*c.args, visible=vis))


def _with_phantom_queries(c, clamped, n=62):
    """rows 130 .. 191 of the ragged query tile let through the mask, seeing every key: zero-filled as the kernel stages them, or
    carrying the clamped row S - 1; lse = D = 0 either way (o = 0)"""
    q, k, v, dO, o, lse, slopes = c.args
    S = q.shape[1]
    ext = lambda t, fill: torch.cat((t, (t[:, S - 1:S] if fill else torch.zeros_like(t[:, :1])).expand(-1, n, *t.shape[2:])), dim=1)
    vis = torch.cat((R._causal(S, S), torch.ones((n, S), dtype=torch.bool)), dim=0)
    return (ext(q, clamped), k, v, ext(dO, clamped), ext(o, False), ext(lse, False), slopes), vis, S


def _with_phantom_keys(c, clamped, n=62):
    """keys 130 .. 191 of the ragged key tile let through the mask for the last query"""
    q, k, v, dO, o, lse, slopes = c.args
    S = q.shape[1]
    ext = lambda t: torch.cat((t, (t[:, S - 1:S] if clamped else torch.zeros_like(t[:, :1])).expand(-1, n, -1)), dim=1)
    vis = torch.cat((R._causal(S, S), torch.zeros((S, n), dtype=torch.bool)), dim=1)
    vis[S - 1, S:] = True
    return (q, ext(k), ext(v), dO, o, lse, slopes), vis, S


def test_phantom_query_rows_are_rejected():
    c = _case(BASE)
    args, vis, S = _with_phantom_queries(c, clamped=True)
    _rejected("query rows >= S contribute (lse = 0)", c, R.emulate(*args, visible=vis, total=S))


def test_phantom_keys_are_rejected():
    c = _case(BASE)
    args, vis, S = _with_phantom_keys(c, clamped=True)
    assert "dq" in _rejected("keys >= S contribute", c, R.emulate(*args, visible=vis, total=S))


def test_zero_filled_phantom_rows_are_harmless():
    """see the module docstring: the zero fill of the ragged tile makes a lost `< S` test invisible, so it cannot be asked for"""
    c = _case(BASE)
    good = R.emulate(*c.args)
    for build in (_with_phantom_queries, _with_phantom_keys):
        args, vis, S = build(c, clamped=False)
        got = R.emulate(*args, visible=vis, total=S)
        for name in ("dq", "dk", "dv"):
            assert torch.equal(got[name][:, :S], good[name]), (build.__name__, name)


def test_d_from_the_neighbouring_row_is_rejected():
    c = _case(BASE)
    _rejected("D of row i + 1", c, R.emulate(*c.args, d_shift=1))


def test_dk_without_scale_is_rejected():
    c = _case(BASE)
    assert _rejected("dK without scale", c, R.emulate(*c.args, dk_scale=False)) == ["dk"]


def test_middle_tile_twice_is_rejected():
    c = _case(ODD_PAIRED)
    assert R.backward_rule(*ODD_PAIRED[:3]).middle
    assert _rejected("middle tile twice", c, R.emulate(*c.args, twice=slice(64, 128))) == ["dq", "dk", "dv"]


def test_alibi_bias_from_the_query_is_rejected():
    c = _case(ALIBI)
    R.check("alibi emulation", R.emulate(*c.args), c.ref)
    _rejected("ALiBi bias slope (key - query)", c, R.emulate(*c.args, bias_from_query=True))
