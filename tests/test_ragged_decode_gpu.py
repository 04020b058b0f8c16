"""Ragged decode kernels: llark_attn_decode_rope_bf16_rows (one KV-cache position per sequence) must equal, row by row and bit for
bit, the scalar-position llark_attn_decode_rope_bf16 at the same batch size (same wave count, same summation order); idle slots stay
untouched; llark_decode_advance_rows must pick exactly torch.argmax and keep the slot bookkeeping."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NH, HD = 32, 128
SMAX = 520
POSITIONS = [0, 1, 63, 64, 370, 511, SMAX - 1]


def _tables(smax):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, HD, 2, dtype=torch.float32) / HD))
    freqs = torch.arange(smax, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return freqs.cos().contiguous().cuda(), freqs.sin().contiguous().cuda()


def _state(batch, split, seed, nh=NH, smax=SMAX):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bf = torch.bfloat16
    k = torch.randn((batch, nh, smax, HD), generator=g, device="cuda").to(bf)
    vt = torch.randn((batch, nh, HD, smax), generator=g, device="cuda").to(bf)
    kl = (torch.randn(k.shape, generator=g, device="cuda") * 2 ** -9).to(bf) if split else None
    vl = (torch.randn(vt.shape, generator=g, device="cuda") * 2 ** -9).to(bf) if split else None
    qkv = torch.randn((batch, 3 * nh * HD), generator=g, device="cuda")
    return qkv, [k, vt, kl, vl]


def _clone(caches):
    return [c.clone() if c is not None else None for c in caches]


def _bits(t):
    return t.view(torch.int16)


def _run_rows(qkv, caches, pos_rows, cos, sin, split, alibi=None):
    from llark_amd import ops
    batch = qkv.shape[0]
    c = _clone(caches)
    out = torch.full((batch, NH * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    out_lo = torch.full_like(out, 7.0) if split else None
    ops.attn_decode_rope_rows(qkv, batch, NH, HD, torch.tensor(pos_rows, dtype=torch.int32, device="cuda"), cos, sin, c[0], c[1], out,
                              c[2], c[3], out_lo, alibi)
    return out, out_lo, c


def _run_scalar(qkv, caches, p, cos, sin, split, alibi=None):
    from llark_amd import ops
    batch = qkv.shape[0]
    c = _clone(caches)
    out = torch.empty((batch, NH * HD), dtype=torch.bfloat16, device="cuda")
    out_lo = torch.empty_like(out) if split else None
    ops.attn_decode_rope(qkv, batch, NH, HD, p, cos, sin, c[0], c[1], out, c[2], c[3], out_lo, alibi)
    return out, out_lo, c


def _check_rows_equal_scalar(batch, split, pos_rows, alibi=None, seed=0):
    cos, sin = _tables(SMAX)
    qkv, caches = _state(batch, split, seed)
    out_r, lo_r, c_r = _run_rows(qkv, caches, pos_rows, cos, sin, split, alibi)
    for p in sorted(set(q for q in pos_rows if q >= 0)):
        out_p, lo_p, c_p = _run_scalar(qkv, caches, p, cos, sin, split, alibi)
        for b in (b for b in range(batch) if pos_rows[b] == p):
            assert torch.equal(_bits(out_r[b]), _bits(out_p[b])), f"row {b} (pos {p}): output head differs"
            if split:
                assert torch.equal(_bits(lo_r[b]), _bits(lo_p[b])), f"row {b} (pos {p}): output lo plane differs"
            for name, x, y in zip(("k", "vt", "k_lo", "vt_lo"), c_r, c_p):
                if x is not None:
                    assert torch.equal(_bits(x[b]), _bits(y[b])), f"row {b} (pos {p}): {name} cache slot differs"
    torch.cuda.synchronize()


@pytest.mark.parametrize("split", [True, False], ids=["split", "bf16"])
@pytest.mark.parametrize("batch", [1, 3, 8, 16])
def test_rows_kernel_equals_scalar_position_kernel(batch, split):
    """Each row of the ragged launch is bit-identical to that row of the scalar launch at p = pos_rows[b] (same batch size: nh * batch
    = 32, 96 < 256 and 256, 512 cross the wave-count switch of attn_decode() in csrc/llama.hip)."""
    if batch == 1:
        for i, p in enumerate(POSITIONS):
            _check_rows_equal_scalar(1, split, [p], seed=i)
    else:
        pos_rows = [POSITIONS[(b * 3 + batch) % len(POSITIONS)] for b in range(batch)]
        assert len(set(pos_rows)) >= min(batch, 3)
        _check_rows_equal_scalar(batch, split, pos_rows, seed=batch)


def test_rows_kernel_alibi_equals_scalar():
    slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / NH) for h in range(NH)], dtype=torch.float32, device="cuda")
    _check_rows_equal_scalar(3, True, [370, 0, SMAX - 1], alibi=slopes, seed=11)
    _check_rows_equal_scalar(8, False, [POSITIONS[b % len(POSITIONS)] for b in range(8)], alibi=slopes, seed=12)


@pytest.mark.parametrize("split", [True, False], ids=["split", "bf16"])
def test_idle_rows_untouched_and_zero(split):
    batch = 5
    pos_rows = [-1, 64, -1, 511, -7]
    cos, sin = _tables(SMAX)
    qkv, caches = _state(batch, split, 3)
    out_r, lo_r, c_r = _run_rows(qkv, caches, pos_rows, cos, sin, split)
    for b in range(batch):
        if pos_rows[b] < 0:
            assert not out_r[b].float().any(), f"idle row {b}: output not zero"
            if split:
                assert not lo_r[b].float().any(), f"idle row {b}: output lo plane not zero"
            for x, y in zip(c_r, caches):
                if x is not None:
                    assert torch.equal(_bits(x[b]), _bits(y[b])), f"idle row {b}: cache slot changed"
    # the active rows next to them are still the scalar kernel's rows
    _check_rows_equal_scalar(batch, split, pos_rows, seed=3)


@pytest.mark.parametrize("split", [True, False], ids=["split", "bf16"])
def test_decode_forms_agree_beyond_the_default_lds_limit(split):
    """smax = 12296 keys: 4 * 12296 bytes of scores is the first multiple-of-8 cache length whose dynamic LDS exceeds the 48 KiB a kernel
    gets by default, so every entry point has to raise its limit on first use -- the host position (LDS sized from the 12291 visible
    keys, rounded up to 8) as well as the device positions (sized from smax).  Position 12290, one sequence, two heads.  The five decode
    forms, each used here for the first time in this order, leave bit-identical output heads and bit-identical caches."""
    from llark_amd import ops
    nh, smax, p, bf = 2, 12296, 12290, torch.bfloat16
    assert 4 * smax > 48 * 1024 >= 4 * (smax - 8) and 4 * ((p + 1 + 7) // 8 * 8) > 48 * 1024
    cos, sin = _tables(smax)
    qkv, caches = _state(1, split, 21, nh=nh, smax=smax)
    pos_dev = torch.tensor([p], dtype=torch.int32, device="cuda")

    def outputs():
        out = torch.full((1, nh * HD), 7.0, dtype=bf, device="cuda")
        return out, (torch.full_like(out, 7.0) if split else None)

    def fused(fn, pos):
        c, (out, out_lo) = _clone(caches), outputs()
        fn(qkv, 1, nh, HD, pos, cos, sin, c[0], c[1], out, c[2], c[3], out_lo)
        return out, out_lo, c

    def unfused(dpos):
        c, (out, out_lo) = _clone(caches), outputs()
        q = torch.empty((1, nh, 1, HD), dtype=bf, device="cuda")
        q_lo = torch.empty_like(q) if split else None
        if dpos:
            ops.rope_split_heads_dpos(qkv, 1, nh, HD, pos_dev, cos, sin, q, c[0], c[1], q_lo, c[2], c[3])
            ops.attn_decode_dpos(q, c[0], c[1], 1, nh, HD, pos_dev, out, q_lo, c[2], c[3], out_lo)
        else:
            ops.rope_split_heads(qkv, 1, 1, nh, HD, p, cos, sin, q, c[0], c[1], q_lo, c[2], c[3])
            ops.attn_decode(q, c[0], c[1], 1, nh, HD, p + 1, out, q_lo, c[2], c[3], out_lo)
        return out, out_lo, c

    runs = [("attn_decode_rope, host position", fused(ops.attn_decode_rope, p)),
            ("attn_decode_rope, device position", fused(ops.attn_decode_rope, pos_dev)),
            ("attn_decode_rope_rows", fused(ops.attn_decode_rope_rows, pos_dev)),
            ("rope_split_heads + attn_decode", unfused(False)),
            ("rope_split_heads_dpos + attn_decode_dpos", unfused(True))]
    torch.cuda.synchronize()
    ref_name, (ref_out, ref_lo, ref_c) = runs[0]
    assert ref_out.float().isfinite().all() and (ref_out.float() != 7.0).any()
    assert not torch.equal(_bits(ref_c[0][0, :, p]), _bits(caches[0][0, :, p])), "the new key row was not written"
    assert not torch.equal(_bits(ref_c[1][0, :, :, p]), _bits(caches[1][0, :, :, p])), "the new value column was not written"
    for name, (out, out_lo, c) in runs[1:]:
        assert torch.equal(_bits(out), _bits(ref_out)), f"{name}: output differs from {ref_name}"
        if split:
            assert torch.equal(_bits(out_lo), _bits(ref_lo)), f"{name}: output lo plane differs from {ref_name}"
        for cname, x, y in zip(("k", "vt", "k_lo", "vt_lo"), c, ref_c):
            if x is not None:
                assert torch.equal(_bits(x), _bits(y)), f"{name}: {cname} cache differs from {ref_name}"


def test_decode_advance_rows_matches_argmax_and_bookkeeping():
    from llark_amd import ops
    A, F, I = ops.ROW_ACTIVE, ops.ROW_FINISHED, ops.ROW_IDLE
    B, V, LD = 8, 1000, 1024
    g = torch.Generator().manual_seed(5)
    buf = torch.randn((B, LD), generator=g)
    buf[:, V:] = 1e9                                        # columns beyond the vocabulary are never read
    buf[0, 5] = buf[0, 700] = 50.0                          # exact tie: the first index wins
    buf[1, :V] = -float("inf")                              # all -inf: index 0, as torch.argmax
    buf[2, : V // 2] = -float("inf")
    buf[2, 999] = buf[2, 600] = buf[2, 601] = 9.0
    buf[3, 17] = 99.0                                       # finished row: emits pad whatever its logits
    buf[6, 123] = 80.0                                      # this row's greedy token is eos -> finished
    buf[7, 42] = float("nan")                               # NaN counts as the maximum (torch semantics)
    state = torch.tensor([A, A, A, F, I, A, A, A], dtype=torch.int32)
    pos = torch.tensor([3, 4, 5, 6, -1, 7, 8, 0], dtype=torch.int32)
    ref = buf[:, :V].argmax(-1)
    assert ref[0] == 5 and ref[1] == 0 and ref[2] == 600 and ref[6] == 123 and ref[7] == 42
    eos, pad = 123, 31
    logits = buf.cuda()[:, :V]
    st, ps = state.cuda(), pos.cuda()
    nxt = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    out = torch.full((B, 10), -9, dtype=torch.int64, device="cuda")
    ops.decode_advance_rows(logits, st, nxt, ps, out[:, 4], eos, pad)
    act = state == A
    want = torch.where(act, ref, torch.full_like(ref, pad))
    assert torch.equal(nxt.cpu(), want) and torch.equal(out[:, 4].cpu(), want)
    keep = torch.ones(10, dtype=torch.bool)
    keep[4] = False
    assert (out.cpu()[:, keep] == -9).all()
    assert torch.equal(ps.cpu(), torch.where(act, pos + 1, pos))
    assert st.cpu().tolist() == [A, A, A, F, I, A, F, A]
    # given tokens (sampling) instead of the argmax; no position array = no advance; eos < 0 = no finishing
    choice = torch.tensor([9, 8, 7, 6, 5, 4, 3, 2], dtype=torch.int64, device="cuda")
    st2 = state.cuda()
    ops.decode_advance_rows(None, st2, nxt, None, None, eos=-1, pad=pad, choice=choice, vocab=V)
    assert nxt.cpu().tolist() == [9, 8, 7, pad, pad, 4, 3, 2] and torch.equal(st2.cpu(), state)
