"""The shared-prefix decode kernels of csrc/attn_shared.hip -- attn_group_kernel + attn_slot_kernel behind
ops.attn_decode_rope_shared, kv_copy_prefix_kernel behind ops.kv_copy_prefix -- against the float64 reference of
tests/llama_kernel_ref.py, with the harness of tests/test_llama_kernels_gpu.py: outputs inside sentinel slabs, the largest finite
bf16 (0x7F7F) in every cache plane at and beyond each slot's ``total``, whole caches and ``qkv`` compared bit for bit with their
expected state after the launch, PLANTED keys (``k_j += 0.6 q``: probability ~0.9).

A scene is a list of slots, each at its own position, and groups (source slot, shared length P, members).  The members' caches hold
copies of the source's positions [0, P).  Planted keys in the shared positions -- 0, 7 | 8, both sides of every round boundary of the
group pass (GK_KEYS = 128 keys per round), P - 8 and P - 1 -- are each planted for ONE member's query (round robin: the keys are
shared, the queries are not); in a member's own positions P (the first key of the per-slot pass), total - 2 and the appended key
total - 1 are planted.  Losing, doubling or misplacing one of them, or merging a partial with the wrong weight, moves all 128
outputs of a head by O(1).

Tolerance: llama_kernel_ref.check_out(..., "decode" | "decode_split", ...) as it stands, ``u + c 2^-24 (1 + 2A) B``.  The scores are
the rows form's own (same fma chain, same shuffle tree); what the shared path adds per output is, per key range and per round, one
expf and one multiplication for the rescaling of the running sums, and in the merge one expf, one multiplication and one fma per
partial (at most GK_SPLITS + 1 = 5 of them) and one reciprocal: a few dozen fp32 roundings next to the ``total``-term fma chains the
bound already covers with c = 16.

Case ids name the kernel's constants: ``r128`` = a round boundary of the group pass (GK_KEYS), ``s512`` = the shared length from which
a key range holds more than one round (GK_KEYS * GK_SPLITS: the running maximum is carried from round to round), ``<16,4>`` / ``<4,8>``
the per-slot pass's waves and loads in flight (it switches at nh * batch = 256, like attn_decode_kernel).

Measured on the MI355X (``-s`` prints every slot of every case as "[ratio] ..."):

    case family                                   kernel / tolerance (worst grouped slot)
    bf16, <16,4>, groups of 1 | 2 | 16            0.97 | 0.97 | 0.98
    split, <16,4>, groups of 1 | 2 | 16           0.11 | 0.13 | 0.14
    <4,8>, bf16 | split                           0.99 | 0.15
    mixed launch nh = 2, bf16 | split             0.96 | 0.13
    mixed launch nh = 32, bf16 | split            0.98 | 0.14
    ungrouped slots of the same launches          0.98 | 0.13    (the rows form's bits)

torch's own float32 ratio r stayed below 4 (c = 16) in every case.  A single bf16 plane sits at 0.96 .. 1.00 of its tolerance by
construction (tests/test_llama_kernels_gpu.py); what the shared path adds shows in the split rows, next to 0.14 .. 0.15 for the
existing decode forms.  The whole file: 103 cases in 7 s on the MI355X.
"""
import functools

import pytest
import torch

import llama_kernel_ref as R
from kernel_util import assert_untouched as _assert_untouched, bits as _bits, gen as _gen, out_slab as _out_slab

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = R.HD
BF = torch.bfloat16
PAD = 8
ERR_INVALID, ERR_UNSUPPORTED = -1, -2             # include/llark_hip.h
GK_KEYS, GK_SPLITS, GK_MEMBERS = 128, 4, 16       # csrc/attn_shared.hip
SMAX = 1048                                       # nh = 2 scenes: 9 rounds at P = smax - 8 (key ranges of 2, 2, 2 and 3 rounds)
SMAX_4W = 264                                     # nh = 32 scenes (the 4-wave per-slot pass: 128 keys per K round)


def _ops():
    from llark_amd import ops
    return ops


def _lib():
    from llark_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_dev(name, a, b):
    w = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.view(w), b.view(w)), f"{name}: {int((a.view(w) != b.view(w)).sum())} elements differ"


class _Out:
    def __init__(self, n, dtype=BF):
        self.host, self.mask = _out_slab(n, dtype, front=PAD, back=PAD)
        self.dev = self.host.to(DEV)
        self.view = self.dev[PAD:PAD + n]

    def result(self, name):
        _assert_untouched(name, self.dev, self.host, self.mask)
        return self.dev.cpu()[PAD:PAD + int(self.mask.sum())]


def _shared_plants(P):
    keys = {0, 7, 8, P - 8, P - 1} | {b + o for b in range(GK_KEYS, P + 1, GK_KEYS) for o in (-1, 0)}
    return sorted(j for j in keys if 0 <= j < P)


class _Scene:
    """pos[b]: position of slot b's new token (< 0 or >= smax: idle); groups: (source slot, P, member slots)"""

    def __init__(self, nh, split, smax, pos, groups, seed):
        self.nh, self.split, self.smax, self.pos, self.groups = nh, split, smax, list(pos), groups
        batch = self.batch = len(pos)
        g = _gen(nh, batch, seed)
        kb = torch.randn(batch, nh, smax, HD, generator=g) * 1.5
        vb = torch.randn(batch, nh, smax, HD, generator=g)
        self.qraw = torch.randn(batch, nh, HD, generator=g) * 1.5
        self.cos, self.sin = R.rope_tables(smax)
        self.live = [b for b in range(batch) if 0 <= pos[b] < smax]
        qrot = torch.zeros(batch, nh, HD)
        for b in self.live:
            qrot[b] = R.rope(self.qraw[b], self.cos[pos[b]], self.sin[pos[b]], torch.float32)
        self.shared = [0] * batch
        for src, P, members in groups:
            for i, j in enumerate(_shared_plants(P)):                     # planted in the source, for one member each
                kb[src, :, j] += R.PLANT * qrot[members[i % len(members)]]
            for m in members:
                self.shared[m] = P
                if m != src:
                    kb[m, :, :P], vb[m, :, :P] = kb[src, :, :P], vb[src, :, :P]
        kraw = torch.zeros(batch, nh, HD)
        for b in self.live:
            p, P = pos[b], self.shared[b]
            own = [j for j in ({P, p - 1} if P else set(R.decode_plants(p + 1))) if P <= j < p]
            for j in own:
                kb[b, :, j] += R.PLANT * qrot[b]
            kraw[b] = kb[b, :, p] + R.PLANT * self.qraw[b]                 # planted before the rotation (linear)
            kb[b, :, p] = R.rope(kraw[b], self.cos[p], self.sin[p], torch.float32)
        cut = R.planes if split else (lambda x: (x.bfloat16(), None))
        kp, vp = cut(kb), cut(vb)
        gar = R.garbage((1,))
        for b in self.live:
            for pl in kp + vp:
                if pl is not None:
                    pl[b, :, pos[b] + 1:] = gar
        self.k_fin = [None if p is None else p.to(DEV) for p in kp]
        self.vt_fin = [None if p is None else p.transpose(2, 3).contiguous().to(DEV) for p in vp]
        self.k_pre = [None if p is None else p.clone() for p in self.k_fin]
        self.vt_pre = [None if p is None else p.clone() for p in self.vt_fin]
        for b in self.live:
            for i in range(2):
                if self.k_pre[i] is not None:
                    self.k_pre[i][b, :, pos[b]] = gar.to(DEV)
                    self.vt_pre[i][b, :, :, pos[b]] = gar.to(DEV)
        self.qkv = torch.cat((self.qraw.view(batch, nh * HD), kraw.view(batch, nh * HD),
                              torch.stack([vb[b, :, max(0, min(pos[b], smax - 1))] for b in range(batch)]).view(batch, nh * HD)), dim=1).contiguous()
        q64 = R.value(*cut(qrot))
        k64, v64 = R.value(*kp), R.value(*vp)
        self.refs = {b: R.reference(q64[b][:, None, :], k64[b, :, :pos[b] + 1], v64[b, :, :pos[b] + 1], pos[b]) for b in self.live}
        self.d_cos, self.d_sin = self.cos.to(DEV), self.sin.to(DEV)

    def tables(self, groups=None, shared=None):
        ops = _ops()
        groups = self.groups if groups is None else groups
        tab = torch.zeros((max(1, len(groups)), ops.SHARED_GROUP_STRIDE), dtype=torch.int32)
        for i, (src, P, members) in enumerate(groups):
            tab[i, 0], tab[i, 1], tab[i, 2] = src, P, len(members)
            for j, m in enumerate(members[:GK_MEMBERS]):
                tab[i, 3 + j] = m
        return (tab[:len(groups)].to(DEV) if groups else None), torch.tensor(self.shared if shared is None else shared, dtype=torch.int32, device=DEV)

    def run(self, form, groups=None, shared=None, pos=None, check_table=True):
        """one launch from the state before the step: (out, out_lo as _Out, k planes, v^T planes, qkv)"""
        ops = _ops()
        batch, nh, split = self.batch, self.nh, self.split
        n_out = batch * nh * HD
        out, out_lo = _Out(n_out), (_Out(n_out) if split else None)
        o2, ol2 = out.view.view(batch, nh * HD), (out_lo.view.view(batch, nh * HD) if split else None)
        k, vt = [None if p is None else p.clone() for p in self.k_pre], [None if p is None else p.clone() for p in self.vt_pre]
        qkv = self.qkv.to(DEV)
        rows = torch.tensor(self.pos if pos is None else pos, dtype=torch.int32, device=DEV)
        if form == "rows":
            ops.attn_decode_rope_rows(qkv, batch, nh, HD, rows, self.d_cos, self.d_sin, k[0], vt[0], o2, k[1], vt[1], ol2)
        else:
            tab, sh = self.tables(groups, shared)
            scratch = torch.zeros(ops.attn_decode_shared_scratch_bytes(batch, nh) // 4, dtype=torch.float32, device=DEV)
            ops.attn_decode_rope_shared(qkv, batch, nh, HD, rows, self.d_cos, self.d_sin, k[0], vt[0], o2, tab, sh, scratch, k[1], vt[1], ol2,
                                        check_table=check_table)
        torch.cuda.synchronize()
        return out, out_lo, k, vt, qkv

    def check(self, name):
        """the shared form against the reference, the expected caches and the rows form"""
        out, out_lo, k, vt, qkv = self.run("shared")
        _same_dev(f"{name} qkv", qkv, self.qkv.to(DEV))
        for i in range(2):
            if k[i] is not None:                          # appended rows bit-equal to torch's rotation, everything else untouched
                _same_dev(f"{name} k cache plane {i}", k[i], self.k_fin[i])
                _same_dev(f"{name} v^T cache plane {i}", vt[i], self.vt_fin[i])
        batch, nh = self.batch, self.nh
        got_hi = out.result(f"{name} out").view(batch, nh, HD)
        got_lo = out_lo.result(f"{name} out_lo").view(batch, nh, HD) if self.split else None
        got = got_hi.double() if got_lo is None else got_hi.double() + got_lo.double()
        for b in range(batch):
            if b in self.live:
                R.check_out(f"{name} slot {b} pos {self.pos[b]} shared {self.shared[b]}", "decode_split" if self.split else "decode",
                            got[b][:, None, :], self.refs[b])
            else:
                assert bool((got[b] == 0).all()), f"{name}: idle slot {b} is not zero"
        r_out, r_lo, rk, rvt, _ = self.run("rows")
        for i in range(2):
            if k[i] is not None:                          # what the rows form appends, and nothing else
                _same_dev(f"{name} k cache plane {i} against the rows form", k[i], rk[i])
                _same_dev(f"{name} v^T cache plane {i} against the rows form", vt[i], rvt[i])
        rows_hi = r_out.result("rows out").view(batch, nh, HD)
        rows_lo = r_lo.result("rows out_lo").view(batch, nh, HD) if self.split else None
        for b in range(batch):
            if self.shared[b] == 0:
                assert torch.equal(_bits(got_hi[b]), _bits(rows_hi[b])), f"{name}: ungrouped slot {b} differs from the rows form"
                if self.split:
                    assert torch.equal(_bits(got_lo[b]), _bits(rows_lo[b])), f"{name}: ungrouped slot {b} lo plane differs from the rows form"


# ---- one group: shared lengths x tails x group sizes --------------------------------------------------------------------------
def _waves(nh, batch):
    return "<16,4>" if nh * batch < 256 else "<4,8>"


def _p_cases(smax):
    named = [(8, "P8"), (16, "P16")]
    for b in (GK_KEYS, GK_KEYS * GK_SPLITS, 2 * GK_KEYS * GK_SPLITS):
        tag = f"r{b}" if b == GK_KEYS else f"s{b}"
        named += [(b - 8, f"{tag}-8"), (b, tag), (b + 8, f"{tag}+8")]
    named.append((smax - 8, "smax-8"))
    return [(p, n) for p, n in named if p <= smax - 8]


def _tails(P, smax, k_round):
    """total - P of member i: 1 (only the appended token), 7, 8, 9 and one crossing a K round of the per-slot pass, then other small
    ones: every member of a group of 16 at a total of its own (at P = smax - 8 only eight tails fit: two members per total)"""
    return [t for t in [1, 7, 8, 9, k_round + 4, 2, 15, 3, 4, 5, 6] + list(range(10, 15)) + list(range(16, 21)) if P + t <= smax]


GROUP_CASES = [pytest.param(2, split, G, P, id=f"{'split' if split else 'bf16'}-nh2-{_waves(2, max(G, 2))}-G{G}-{name}")
               for split in (False, True) for G in (1, 2, GK_MEMBERS) for P, name in _p_cases(SMAX)]


@pytest.mark.parametrize("nh,split,G,P", GROUP_CASES)
def test_shared_group(nh, split, G, P):
    """a key lost or doubled at a round or key-range boundary of the group pass, at P - 1 | P between the two passes, a partial of
    another member or head, a wrong weight in the merge, the rescaling of the running sums"""
    smax = SMAX
    tails = _tails(P, smax, 256)
    batch = max(G, 2)                                           # groups of 1: a second, ungrouped slot next to it
    members = list(range(G))
    pos = [P + tails[i % len(tails)] - 1 for i in range(G)] + [P + 3] * (batch - G)
    src = members[len(members) // 2]                            # not the lowest member
    _Scene(nh, split, smax, pos, [(src, P, members)], seed=P).check(f"shared nh{nh} G{G} P{P}")


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("P,name", [(8, "P8"), (GK_KEYS - 8, "r128-8"), (GK_KEYS, "r128"), (GK_KEYS + 8, "r128+8"), (SMAX_4W - 8, "smax-8")])
def test_shared_group_4_waves(P, name, split):
    """nh * batch = 256: the per-slot pass on 4 waves, 128 keys per K round (a tail of 132 crosses it)"""
    nh, smax = 32, SMAX_4W
    tails = _tails(P, smax, 128)
    members = [0, 1, 2, 4, 5]
    pos = [0] * 8
    for i, m in enumerate(members):
        pos[m] = P + tails[i % len(tails)] - 1
    pos[3], pos[6], pos[7] = 140, P + 6, P + 1
    _Scene(nh, split, smax, pos, [(0, P, members), (7, P, [6, 7])], seed=P + 1).check(f"shared <4,8> P{P}")


def _mixed(nh):
    smax = SMAX_4W
    #        0    1    2    3   4    5     6   7    8    9   10   11
    pos = [200, 136, -1, 40, 150, smax, 16, 263, 77, 23, 0, 139]
    groups = [(1, 136, [1, 4, 7]), (6, 16, [9, 3, 6])]         # source = lowest member | source not in slot order
    return smax, pos, groups


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("nh", [2, 32], ids=["nh2-<16,4>", "nh32-<4,8>"])
def test_shared_mixed_launch(nh, split):
    """two groups with different P, ungrouped slots, an idle slot, a slot at smax, sources in and out of slot order: a member using
    another group's partial or table row, an ungrouped slot that is not the rows form bit for bit"""
    smax, pos, groups = _mixed(nh)
    _Scene(nh, split, smax, pos, groups, seed=7).check(f"shared mixed nh{nh}")


def test_shared_without_groups_is_the_rows_form():
    """no group at all (n_groups = 0): every slot bit-equal to attn_decode_rope_rows"""
    _Scene(2, True, SMAX_4W, [5, 130, -1, 263], [], seed=3).check("shared no groups")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _refusal_scene():
    return _Scene(2, False, SMAX_4W, [100, 90, 80, -1] + [70] * 14, [(0, 64, [0, 1, 2])], seed=5)


@pytest.mark.parametrize("case,groups,shared,code", [
    ("P%8", [(0, 60, [0, 1, 2])], [60, 60, 60] + [0] * 15, 1),
    ("group of 17", [(0, 64, [0, 1, 2] + list(range(4, 18)))], [64, 64, 64, 0] + [64] * 14, 2),
    ("P > member position", [(0, 88, [0, 1, 2])], [88, 88, 88] + [0] * 15, 3),
    ("idle source", [(3, 64, [0, 1, 2])], [64, 64, 64] + [0] * 15, 4),
])
def test_shared_refuses(case, groups, shared, code):
    """the table is device data: the kernel refuses through the status word (and forms no address from the refused entries)"""
    ops = _ops()
    S = _refusal_scene()
    with pytest.raises(ops._lib.LlarkHipError, match=f"status {code}"):
        S.run("shared", groups=groups, shared=shared)


def test_shared_host_refusals():
    L, ops = _lib(), _ops()
    batch, nh, smax = 2, 2, 16
    qkv = torch.zeros((batch, 3 * nh * HD), dtype=torch.float32, device=DEV)
    k = torch.zeros((batch, nh, smax, HD), dtype=BF, device=DEV)
    vt = torch.zeros((batch, nh, HD, smax), dtype=BF, device=DEV)
    out = torch.zeros((batch, nh * HD), dtype=BF, device=DEV)
    cos, sin = (t.to(DEV) for t in R.rope_tables(smax))
    rows = torch.full((batch,), -1, dtype=torch.int32, device=DEV)
    sh = torch.zeros(batch, dtype=torch.int32, device=DEV)
    tab = torch.zeros((3, ops.SHARED_GROUP_STRIDE), dtype=torch.int32, device=DEV)
    nbytes = ops.attn_decode_shared_scratch_bytes(batch, nh)
    assert nbytes == 64 + batch * nh * GK_SPLITS * 132 * 4
    sc = torch.zeros(nbytes // 4, dtype=torch.float32, device=DEV)
    p = lambda t: t.data_ptr()
    call = lambda hd, ng, nb: L.llark_attn_decode_rope_bf16_shared(p(qkv), batch, nh, hd, p(rows), p(cos), p(sin), smax, p(k), p(vt), None, None, smax,
                                                                   p(out), None, p(tab), ng, p(sh), p(sc), nb, _stream())
    assert call(64, 0, nbytes) == ERR_UNSUPPORTED               # head_dim
    assert call(HD, 3, nbytes) == ERR_UNSUPPORTED               # more groups than slots
    assert call(HD, 0, nbytes - 4) == ERR_INVALID               # scratch too small
    assert call(HD, 0, nbytes) == 0
    with pytest.raises(ops._lib.LlarkHipError):
        ops.attn_decode_rope_shared(qkv.cpu(), batch, nh, HD, rows, cos, sin, k, vt, out, None, sh, sc)
    torch.cuda.synchronize()


# ---- kv_copy_prefix -----------------------------------------------------------------------------------------------------------
COPY_SMAX = 24


def _copy_planes(split, seed):
    g = _gen(seed, 77)
    layers, slots, nh = 2, 5, 2
    mk = lambda shape: torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int32).to(torch.int16)
    k = [mk((layers, slots, nh, COPY_SMAX, HD)) for _ in range(2 if split else 1)]
    vt = [mk((layers, slots, nh, HD, COPY_SMAX)) for _ in range(2 if split else 1)]
    return k, vt


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, COPY_SMAX])
def test_kv_copy_prefix(n, split):
    """dst[0:n) bit-equal to src in every layer, head and plane; nothing at or beyond round_up(n, 8) and no other slot written"""
    ops = _ops()
    k0, vt0 = _copy_planes(split, n)
    src, dst = 2, [4, 1]
    k = [t.to(DEV).view(BF) for t in k0] + [None] * (2 - len(k0))
    vt = [t.to(DEV).view(BF) for t in vt0] + [None] * (2 - len(vt0))
    ops.kv_copy_prefix(k[0], vt[0], src, dst, n, k[1], vt[1])
    torch.cuda.synchronize()
    up = R.round_up(n, 8)
    for i in range(len(k0)):
        ka, va = k[i].view(torch.int16).cpu(), vt[i].view(torch.int16).cpu()
        for s in range(5):
            if s in dst:
                assert torch.equal(ka[:, s, :, :n], k0[i][:, src, :, :n]) and torch.equal(va[:, s, :, :, :n], vt0[i][:, src, :, :, :n]), f"plane {i} slot {s}"
                assert torch.equal(ka[:, s, :, n:], k0[i][:, s, :, n:]), f"K plane {i} slot {s}: written beyond n"
                assert torch.equal(va[:, s, :, :, up:], vt0[i][:, s, :, :, up:]), f"V^T plane {i} slot {s}: written beyond round_up(n, 8)"
            else:
                assert torch.equal(ka[:, s], k0[i][:, s]) and torch.equal(va[:, s], vt0[i][:, s]), f"plane {i}: slot {s} was written"


def test_kv_copy_prefix_refusals():
    L, ops = _lib(), _ops()
    import ctypes
    k0, vt0 = _copy_planes(False, 0)
    k, vt = k0[0].to(DEV).view(BF), vt0[0].to(DEV).view(BF)

    def call(src, dst, n):
        arr = (ctypes.c_int * len(dst))(*dst)
        return L.llark_kv_copy_prefix(k.data_ptr(), vt.data_ptr(), None, None, 2, 5, 2, HD, COPY_SMAX, src, ctypes.cast(arr, ctypes.c_void_p), len(dst), n,
                                      _stream())
    assert call(2, [4, 1], COPY_SMAX + 1) == ERR_UNSUPPORTED    # n > smax
    assert call(2, [4, 2], 8) == ERR_UNSUPPORTED                # src inside dst
    assert call(2, [4, 1, 4], 8) == ERR_UNSUPPORTED             # a slot twice
    assert call(2, [4, 5], 8) == ERR_INVALID                    # a slot outside the cache
    torch.cuda.synchronize()
    assert torch.equal(k.view(torch.int16).cpu(), k0[0]) and torch.equal(vt.view(torch.int16).cpu(), vt0[0])
    with pytest.raises(ops._lib.LlarkHipError):
        ops.kv_copy_prefix(k.cpu(), vt, 2, [1], 8)
