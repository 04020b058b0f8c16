"""The checker of tests/test_prior_kernels_gpu.py has teeth, shown without running a kernel: the float64 reference and the bound of
tests/prior_kernel_ref.py accept the CPU emulation of the documented arithmetic (fp16 hi / lo operands, three products per pair, fp32
softmax, the output split again) and reject CPU stand-ins for wrong kernels, through the same ``check_attn`` the GPU tests call, on
cases a and e at the unit scale and for the pattern a stand-in belongs to.

Two stand-ins exist on one of the two cases only and are asserted absent on the other, not skipped over silently: "key 64 of a 128-key
range dropped" needs a transposed pattern with two chunks (case e; case a has 8 keys), "the other clip's rows used" needs two clips
(case a; case e has one).  At the small scale (q, k 0.05, v 0.02) the dropped P V pass and the dropped output plane are rejected as
well, but the dropped lo.hi pass of the SCORE product cannot be rejected by any bound the format allows and is asserted ACCEPTED: q's
lo plane is below 2^-14 there and holds steps of 2^-24, so what that pass carries (2^-11 of a score of order 0.01) is no more than
what the subnormal lo planes of q and k lose anyway -- the second term of the floor F (it reaches 0.2 .. 0.3 of the tolerance).

Also here: the dense reference equals oracle.jukebox_ref.factored_attention in float64 on every shape of the table (two independent
statements of each pattern), the table reaches every branch of the launcher's rule, and the plants sit on the edges of the visible sets.
"""
import pytest
import torch

import prior_kernel_ref as R

TEETH = ("a", "e")


def _rejected(name, ref, got):
    with pytest.raises(AssertionError):
        R.check_attn(name, got, ref)


def _emu(ref, vis=None, **kw):
    i = ref.inp
    return R.emulate(kw.pop("q", i.q), kw.pop("k", i.k), kw.pop("v", i.v), ref.vis if vis is None else vis, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
def test_launcher_rule_reaches_every_branch():
    rules = {(c, p): R.attn_rule(t, heads, hd, blocks, p) for c, (n, t, heads, hd, blocks) in R.ATTN_CASES.items() for p in R.PATTERNS}
    assert {r.nk32 for r in rules.values()} == {1, 2, 3, 4, 5}
    assert [rules[c, 1].nk32 for c in "abcdefg"] == [1, 2, 3, 4, 5, 5, 1]
    p2 = [r for (c, p), r in rules.items() if p == 2]
    assert {(r.numbering, r.chunks) for r in p2} == {("xcd", 1), ("xcd", 2), ("linear", 1), ("linear", 2)}
    assert {min(r.nkeys, 64) if r.nkeys <= 64 else r.nkeys for r in p2} >= {64, 128} and any(r.nkeys < 64 for r in p2)
    assert (rules["c", 2].nkeys, rules["c", 2].grid_x, rules["c", 2].numbering) == (64, 8, "xcd")
    assert (rules["d", 2].nkeys, rules["d", 2].chunks, rules["d", 2].numbering) == (128, 2, "xcd")
    assert (rules["e", 2].nkeys, rules["e", 2].chunks, rules["e", 2].numbering) == (128, 2, "linear")
    assert rules["b", 1].block_ctx == 34 and rules["g", 1].block_ctx == 1 and rules["a", 1].block_ctx == 64      # ragged, smallest, largest tile
    for c, (n, t, heads, hd, blocks) in R.ATTN_CASES.items():
        S = heads * hd
        assert not R.attn_refused(t, S, heads, blocks, 1, 3 * S + 6, S + 2), c
    assert set(R.LO8_CASES) <= set(R.ATTN_CASES) and ("a", "small") in R.ATTN_RUNS and ("e", "small") in R.ATTN_RUNS
    # the refusals of the GPU file, by the restated rule: (t, n_state, heads, blocks, pattern, ldq, ldo)
    for name, args in R.ATTN_REFUSALS.items():
        assert R.attn_refused(*args), name
    assert not R.attn_refused(512, 48, 2, 8, 1, 150, 50)                # what each of them departs from
    # row kernels: every instantiation of both LayerNorm forms, and of the fused head
    assert {R.ln_rule(w, *R.ln_lds(w)) for w in R.LN8_WIDTHS} == {("8", 1), ("8", 4), ("8", 10), ("8", 16)}
    assert [R.ln_rule(w, *R.ln_lds(w))[1] for w in R.LN8_WIDTHS] == [1, 1, 4, 4, 10, 10, 16, 16]
    assert [R.ln_rule(w, *R.ln_lds(w)) for w in R.LN4_WIDTHS] == [("4", v) for v in (1, 1, 4, 4, 16, 16, 19, 19, 32, 32)]
    assert [R.ln_rule(w, *R.ln_lds(w, forced4=True)) for w in R.LN_FORCED4] == [("4", 4), ("4", 32)]
    assert set(R.LN_LO8_WIDTHS) <= set(R.LN8_WIDTHS + R.LN4_WIDTHS)
    assert {R.ln_rule(w, *R.ln_lds(w)) for w in R.LN_LO8_WIDTHS} >= {("8", 1), ("8", 16), ("4", 1), ("4", 19), ("4", 32)}
    assert R.ln_rule(8200, 8200, 8200) is None and R.ln_rule(8196, 8196, 8196) is None and R.ln_rule(8192, 8192, 8192) == ("8", 16)
    assert [R.head_ng(w) for w in (8, 520, 5128, 8192)] == [1, 4, 16, 16] and R.head_ng(4800) == 10      # NG = 10: tests/test_prior_head_gpu.py


def test_plants_cover_the_edges():
    for case, (n, t, heads, hd, blocks) in R.ATTN_CASES.items():
        bc = t // blocks
        for pattern in R.PATTERNS:
            vis = R.visible(pattern, t, bc)
            plants = R.attn_plants(pattern, n, t, heads, blocks)
            assert len({(p.kc, p.kh, p.j) for p in plants}) == len(plants)
            seen = [p for p in plants if p.kind == "vis"]
            assert seen and len({p.i for p in seen}) == 1 and all((p.qc, p.qh) == (p.kc, p.kh) == (n - 1, heads - 1) for p in seen)
            i = seen[0].i
            keys = torch.nonzero(vis[i]).flatten().tolist()
            assert {keys[0], keys[-1]} <= {p.j for p in seen} <= set(keys), (case, pattern)
            if pattern == 2 and blocks == 128:
                assert len(keys) == 128 and {keys[63], keys[64]} <= {p.j for p in seen}
            masked = [p for p in plants if p.kind == "masked"]
            same = [p for p in masked if (p.kc, p.kh) == (p.qc, p.qh)]
            assert same and all(not vis[p.i, p.j] for p in same)
            why = {p.why for p in masked}
            assert why >= {1: {"next key"}, 2: {"next block"}, 3: {"own block"}}[pattern], (case, pattern, why)
            assert ("block b - 2" in why) == (pattern == 3 and blocks >= 3)
            assert ("other clip" in why) == (n == 2) and ("other head" in why) == (heads >= 2)
            for p in masked:
                if p.why == "next key":
                    assert p.j == p.i + 1 and (bc == 1 or p.j // bc == p.i // bc)
                if p.why == "next block":
                    assert p.j == p.i + bc
                if p.why in ("other clip", "other head"):                         # the position a visible plant has in the query's own rows
                    assert vis[p.i, p.j] and (p.kc, p.kh) != (p.qc, p.qh)


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", list(R.ATTN_CASES))
def test_dense_reference_equals_the_oracle(case, pattern):
    from oracle import jukebox_ref as O
    ref = R.attn_reference(case, pattern)
    i = ref.inp
    S = i.heads * i.hd
    q, k, v = (R.to_rows(x).double().view(i.n, i.t, S).contiguous() for x in (i.q, i.k, i.v))
    want = O.factored_attention(q, k, v, pattern, i.heads, i.bc, dtype=torch.float64)
    got = R.to_rows(ref.out).view(i.n, i.t, S)
    assert float((got - want).abs().max()) <= 1e-12
    if pattern == 3:
        assert not bool(ref.out[:, :, :i.bc].any()) and not bool(ref.bound[:, :, :i.bc].any())
    # the planted keys weigh what they were planted to weigh: a visible plant's row dominates the query's output
    seen = [p for p in i.plants if p.kind == "vis"]
    assert i.hd == 2 or float(ref.out[seen[0].qc, seen[0].qh, seen[0].i].abs().max()) > 1.0       # hd = 2: |q_i|^2 is anything


# ---------------------------------------------------------------------------------------------------------------------
# the emulation is accepted
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case,scale", R.ATTN_RUNS)
def test_emulation_of_the_documented_arithmetic_is_accepted(case, scale, pattern):
    ref = R.attn_reference(case, pattern, scale)
    frac = R.check_attn(f"emulation {case} {scale} pattern {pattern}", ref.emu, ref)
    assert frac <= 0.25 and ref.c >= 4.0
    print(f"[ratio] emulation {case} {scale} pattern {pattern}: {ref.r_rel:.3g} x the bound without its floor F, 2^-22 (1 + 2A) B")
    if scale == "small":
        assert ref.r_rel > 4.0                  # no purely relative bound with c = 4 holds for the format at this scale


# ---------------------------------------------------------------------------------------------------------------------
# wrong kernels are rejected
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", TEETH)
@pytest.mark.parametrize("what", ["drop_qk", "drop_pv", "drop_out_lo"])
def test_a_dropped_pass_or_plane_is_rejected(case, pattern, what):
    ref = R.attn_reference(case, pattern)
    _rejected(f"{what} {case} pattern {pattern}", ref, _emu(ref, **{what: True}))
    small = R.attn_reference(case, pattern, "small")
    got = _emu(small, **{what: True})
    if what == "drop_qk":                                                 # see the module docstring: inside the floor at this scale
        assert R.check_attn(f"{what} {case} small pattern {pattern}", got, small) <= 1.0
    else:
        _rejected(f"{what} {case} small pattern {pattern}", small, got)


@pytest.mark.parametrize("case", TEETH)
def test_causal_mask_one_key_late_is_rejected(case):
    ref = R.attn_reference(case, 1)
    t, bc = ref.inp.t, ref.inp.bc
    i, j = torch.arange(t)[:, None], torch.arange(t)[None, :]
    _rejected("j = i + 1 admitted", ref, _emu(ref, ref.vis | ((j == i + 1) & (j // bc == i // bc))))


@pytest.mark.parametrize("case", TEETH)
def test_transposed_pattern_admitting_the_next_block_is_rejected(case):
    ref = R.attn_reference(case, 2)
    t, bc = ref.inp.t, ref.inp.bc
    i, j = torch.arange(t)[:, None], torch.arange(t)[None, :]
    _rejected("block b + 1 admitted", ref, _emu(ref, (i % bc == j % bc) & (j // bc <= i // bc + 1)))


@pytest.mark.parametrize("case", TEETH)
def test_previous_block_pattern_reading_its_own_block_is_rejected(case):
    ref = R.attn_reference(case, 3)
    t, bc = ref.inp.t, ref.inp.bc
    i, j = torch.arange(t)[:, None], torch.arange(t)[None, :]
    _rejected("own block read", ref, _emu(ref, j // bc == i // bc))


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", TEETH)
def test_a_dropped_visible_plant_is_rejected(case, pattern):
    ref = R.attn_reference(case, pattern)
    for p in (p for p in ref.inp.plants if p.kind == "vis"):
        vis = ref.vis.clone()
        assert vis[p.i, p.j]
        vis[p.i, p.j] = False
        _rejected(f"plant {p.why} dropped", ref, _emu(ref, vis))


@pytest.mark.parametrize("case", TEETH)
def test_an_admitted_masked_plant_is_rejected(case):
    for pattern in R.PATTERNS:
        ref = R.attn_reference(case, pattern)
        for p in (p for p in ref.inp.plants if p.kind == "masked" and (p.kc, p.kh) == (p.qc, p.qh)):
            vis = ref.vis.clone()
            assert not vis[p.i, p.j]
            vis[p.i, p.j] = True
            _rejected(f"plant {p.why} admitted", ref, _emu(ref, vis))


def test_key_64_of_a_128_key_range_dropped_is_rejected():
    assert R.attn_rule(*R.ATTN_CASES["a"][1:], 2).nkeys == 8                    # case a has no such key
    ref = R.attn_reference("e", 2)
    assert R.attn_rule(*R.ATTN_CASES["e"][1:], 2).nkeys == 128
    t, bc = ref.inp.t, ref.inp.bc
    i, j = torch.arange(t)[:, None], torch.arange(t)[None, :]
    _rejected("key 64 dropped", ref, _emu(ref, ref.vis & ~((j // bc == 64) & (i // bc >= 64))))


def test_the_other_clips_rows_are_rejected():
    assert R.ATTN_CASES["e"][0] == 1                                           # case e has one clip
    for pattern in R.PATTERNS:
        ref = R.attn_reference("a", pattern)
        _rejected("other clip", ref, _emu(ref, k=ref.inp.k.flip(0), v=ref.inp.v.flip(0)))
        # ... and the neighbouring head's
        _rejected("other head", ref, _emu(ref, k=ref.inp.k.flip(1), v=ref.inp.v.flip(1)))


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", TEETH)
def test_scale_one_over_head_dim_is_rejected(case, pattern):
    ref = R.attn_reference(case, pattern)
    _rejected("scale 1 / hd", ref, _emu(ref, scale=1.0 / ref.inp.hd))


# ---------------------------------------------------------------------------------------------------------------------
# row kernels: the references' own consistency
# ---------------------------------------------------------------------------------------------------------------------
def test_lo8_positions_are_a_permutation_of_each_64_block():
    pos = R.lo8_pos(torch.arange(192))
    assert sorted(pos.tolist()) == list(range(192)) and all(int(p) // 64 == k // 64 for k, p in enumerate(pos))
    assert [int(R.lo8_pos(k)) for k in (0, 7, 8, 16, 24, 63)] == [0, 7, 32, 8, 40, 63]
    assert int(R.lo8_written(2, 128, 70).sum()) == 140


def test_layernorm_tolerance_rejects_a_dropped_lo_plane_and_accepts_the_planes():
    for data in R.LN_DATA:
        x, gamma, beta = R.ln_inputs(5, 260, data)
        ref, atol, r = R.ln_reference(x, gamma, beta)
        y = torch.nn.functional.layer_norm(x, (260,), gamma, beta, R.LN_EPS)
        hi, lo = R.split16(y)
        R.check_frac(f"fp32 layer_norm as planes, {data}", hi + lo, ref, atol, r)
        if data == "randn":
            with pytest.raises(AssertionError):
                R.check_frac("hi plane alone", hi, ref, atol, r)


@pytest.mark.parametrize("rows", R.PRED_ROWS)
@pytest.mark.parametrize("width", R.PRED_WIDTHS)
def test_ln_row_pred_inputs_keep_their_margin(rows, width):
    x = R.pred_inputs(rows, width)
    assert R.pred_margin(x) >= R.PRED_MARGIN
    l2 = R.pred_reference(x)[2]
    if rows > 1:
        assert len(set(torch.round(l2).tolist())) >= 3                  # rows of different scale
