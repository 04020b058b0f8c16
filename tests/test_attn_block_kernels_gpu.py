"""llark_attn_decode_rope_bf16_block (csrc/attn_block.hip): the out planes of every row and all four cache planes must be BIT-equal to
blk[b] successive llark_attn_decode_rope_bf16_rows launches from identical initial caches (launch i feeds row i of every slot whose block
has one, the other slots idle), in both wave geometries, with bf16 and with hi + lo planes.  Beyond each slot's length the caches hold
random finite bit patterns, the largest magnitudes included: a stale column that reaches a result -- through the ragged last V chunk,
where hi + lo of two stale planes overflows -- shows up as a NaN or a changed bit.  The computed rows are also held to the float64
reference of tests/llama_kernel_ref.py under the bound the decode-attention tests of tests/test_llama_kernels_gpu.py use."""
import pytest
import torch

import llama_kernel_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = R.HD
BF = torch.bfloat16
ERR_INVALID, ERR_UNSUPPORTED = -1, -2             # include/llark_hip.h
SENTINEL = 0x7FC1                                 # a NaN pattern no kernel writes: an output element left unwritten keeps it


def _ops():
    from llark_amd import ops
    return ops


def _bits16(t):
    return t.view(torch.int16)


def _stale(shape, g):
    """random bf16 bit patterns, finite per plane: an all-ones exponent has its lowest exponent bit cleared (-> magnitude ~ 1e38)"""
    b = torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7F80) == 0x7F80, b & ~0x0080, b)
    return b.to(torch.int16).view(BF)


def _caches(n_slots, nh, smax, lens, split, g):
    """[k, vt, k_lo, vt_lo] on the host: values of size ~1 below each slot's length, stale bits at and beyond it"""
    k, v = torch.randn(n_slots, nh, smax, HD, generator=g) * 1.5, torch.randn(n_slots, nh, smax, HD, generator=g)
    planes = []
    for x in (k, v):
        hi, lo = R.planes(x)
        planes.append([hi, lo if split else None])
    out = []
    for i in range(2 if split else 1):
        kp, vp = planes[0][i].clone(), planes[1][i].clone()
        for b, n in enumerate(lens):
            kp[b, :, n:] = _stale((nh, smax - n, HD), g)
            vp[b, :, n:] = _stale((nh, smax - n, HD), g)
        out += [kp.contiguous(), vp.transpose(2, 3).contiguous()]
    return out + [None] * (4 - len(out))


def _check(nh, smax, stride, cases, split, seed, check_ref=True):
    ops = _ops()
    n = len(cases)
    H = nh * HD
    g = torch.Generator().manual_seed(seed)
    pos = [c[0] for c in cases]
    blk = [c[1] for c in cases]
    cos, sin = R.rope_tables(smax)
    qkv = torch.randn(n * stride, 3 * H, generator=g) * 1.5
    host = _caches(n, nh, smax, [max(0, min(p, smax)) for p in pos], split, g)
    d_cos, d_sin, d_qkv = cos.to(DEV), sin.to(DEV), qkv.to(DEV)
    new = lambda: [None if p is None else p.to(DEV) for p in host]
    out_buf = lambda rows: [torch.full((rows, H), SENTINEL, dtype=torch.int16, device=DEV).view(BF) if (i == 0 or split) else None for i in range(2)]

    # the block launch
    A = new()
    outA = out_buf(n * stride)
    ops.attn_decode_rope_block(d_qkv, n, stride, nh, HD, torch.tensor(blk, dtype=torch.int32, device=DEV), torch.tensor(pos, dtype=torch.int32, device=DEV),
                               d_cos, d_sin, A[0], A[1], outA[0], A[2], A[3], outA[1])
    torch.cuda.synchronize()
    assert torch.equal(d_qkv.cpu().view(torch.int32), qkv.view(torch.int32)), "qkv was modified"

    # blk[b] successive rows launches from the same initial caches
    B = new()
    want = [torch.zeros(n * stride, H, dtype=BF) for _ in range(2)]
    steps = max([min(c, stride) for c in blk] + [0])
    for i in range(steps):
        pr = [pos[b] + i if (pos[b] >= 0 and i < blk[b]) else -1 for b in range(n)]
        o = out_buf(n)
        ops.attn_decode_rope_rows(d_qkv.view(n, stride, 3 * H)[:, i].contiguous(), n, nh, HD, torch.tensor(pr, dtype=torch.int32, device=DEV), d_cos, d_sin,
                                  B[0], B[1], o[0], B[2], B[3], o[1])
        torch.cuda.synchronize()
        for b in range(n):
            if pr[b] >= 0:
                for pl in range(2 if split else 1):
                    want[pl][b * stride + i] = o[pl][b].cpu()
    tag = f"nh={nh} smax={smax} stride={stride} {cases} {'split' if split else 'bf16'}"
    for pl in range(2 if split else 1):
        got = outA[pl].cpu()
        diff = _bits16(got) != _bits16(want[pl])
        assert not bool(diff.any()), f"{tag}: out plane {pl}: {int(diff.sum())} elements differ, first rows {sorted(set(diff.nonzero()[:, 0].tolist()))[:8]}"
    for i, name in enumerate(("k", "v^T", "k_lo", "v^T_lo")):
        if A[i] is not None:
            diff = _bits16(A[i]) != _bits16(B[i])
            assert not bool(diff.any()), f"{tag}: cache plane {name}: {int(diff.sum())} elements differ"
    # rows that compute nothing: zeros, and their cache positions untouched (equal to B, which equals the initial state there)
    for b in range(n):
        live = 0 if pos[b] < 0 else max(0, min(blk[b], stride, smax - pos[b]))
        for pl in range(2 if split else 1):
            assert bool((_bits16(outA[pl].cpu()[b * stride + live:(b + 1) * stride]) == 0).all()), f"{tag}: slot {b}: rows >= {live} are not zero"
        if live == 0:
            for i in range(4):
                if A[i] is not None:
                    assert torch.equal(_bits16(A[i][b]).cpu(), _bits16(host[i][b])), f"{tag}: slot {b} computes nothing but cache plane {i} changed"
    if not check_ref:
        return
    # the float64 reference, from the operand values the kernel read: the final caches up to each query's own length
    kf = R.value(A[0].cpu(), None if A[2] is None else A[2].cpu())
    vf = R.value(A[1].cpu(), None if A[3] is None else A[3].cpu()).transpose(2, 3)
    got = R.value(outA[0].cpu(), outA[1].cpu() if split else None).view(n, stride, nh, HD)
    for b in range(n):
        live = 0 if pos[b] < 0 else max(0, min(blk[b], stride, smax - pos[b]))
        for i in sorted({0, live // 2, live - 1}) if live else []:
            p = pos[b] + i
            qraw = qkv[b * stride + i, :H].view(nh, HD)
            q = R.value(*(R.planes(R.rope(qraw, cos[p], sin[p], torch.float32)) if split else (R.rope(qraw, cos[p], sin[p], torch.float32).bfloat16(), None)))
            ref = R.reference(q[:, None, :], kf[b, :, :p + 1], vf[b, :, :p + 1], p)
            R.check_out(f"{tag} slot {b} row {i}", "decode_split" if split else "decode", got[b, i][:, None, :], ref)


SPLIT = pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])


@SPLIT
def test_block_crossing_chunks_first_token_and_end_of_cache(split):
    """totals 6 .. 13 cross a multiple of 8 (every query its own ragged last chunk); the first token (total 1); a block that ends
    exactly at smax"""
    _check(2, 64, 8, [(5, 8), (0, 3), (56, 8)], split, 1)


@SPLIT
def test_block_rows_that_compute_nothing(split):
    """rows at positions >= smax write nothing and give zeros (61 + 3 .. 61 + 7); blk = 0; pos = -1; blk beyond stride counts as
    stride; a position >= smax"""
    _check(2, 64, 8, [(61, 8), (5, 0), (-1, 4)], split, 2)
    _check(2, 64, 8, [(20, 11), (64, 3), (63, 2)], split, 3)


@SPLIT
@pytest.mark.parametrize("stride", [1, 2, 3, 4, 5])
def test_block_strides(stride, split):
    """stride 1 must equal the rows kernel itself; 2, 4 and 8 are compiled capacities, 3 and 5 run inside the next one"""
    _check(2, 64, stride, [(5, stride), (0, 1), (64 - stride, stride), (-1, 1)], split, 10 + stride)


@SPLIT
def test_block_four_wave_geometry(split):
    """nh * n_slots = 256: the 256-thread workgroups, two threads per output dim in the PV pass"""
    _check(32, 64, 8, [(5, 8), (0, 3), (56, 8), (61, 8), (5, 0), (-1, 4), (17, 2), (30, 5)], split, 4)


@SPLIT
def test_block_long_cache_raises_the_lds_limit(split):
    """8 * 1544 * 4 bytes: the first multiple-of-8 length whose scores pass the 48 KiB default of dynamic LDS; totals 1531 .. 1538 also
    walk several rounds of the K and V passes at 16 waves"""
    _check(1, 1544, 8, [(1530, 8)], split, 5)


def test_block_refuses_scores_beyond_128_kib_before_any_launch():
    from llark_amd import _lib
    L = _lib.lib()
    smax, stride, nh = 4104, 8, 1                  # 8 * 4104 * 4 = 131328 > 131072
    z = torch.full((stride, 3 * HD), SENTINEL, dtype=torch.int16, device=DEV)
    i32 = torch.ones(1, dtype=torch.int32, device=DEV)
    p, s = z.data_ptr(), torch.cuda.current_stream().cuda_stream
    args = lambda st, sm: (p, 1, st, nh, HD, i32.data_ptr(), i32.data_ptr(), p, p, sm, p, p, None, None, sm, p, None, s)
    assert L.llark_attn_decode_rope_bf16_block(*args(stride, smax)) == ERR_UNSUPPORTED
    assert b"LDS" in L.llark_last_error()
    assert L.llark_attn_decode_rope_bf16_block(*args(9, 64)) == ERR_INVALID          # stride
    assert L.llark_attn_decode_rope_bf16_block(*args(8, 60)) == ERR_INVALID          # smax % 8
    torch.cuda.synchronize()
    assert bool((z.cpu() == SENTINEL).all()), "a refused call wrote something"
