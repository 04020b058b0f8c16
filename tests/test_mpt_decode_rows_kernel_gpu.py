"""llark_mpt_attn_decode_rows (csrc/llama.hip: mpt_attn_decode_kernel) alone, against float64: the MPT ragged decode step's clamp +
qk_ln + head split + cache append + ALiBi decode attention in one launch.

What is checked, per case (inputs and references from tests/llama_kernel_ref.py, the front from tests/mpt_decode_ref.py):

* the appended K row and V^T column of every active slot, per plane, against the float64 clamp (+ LayerNorm) value rounded to the
  plane(s): bit-exact without qk_ln (a planted NaN must come back a NaN); with qk_ln within the bound of mpt_decode_ref
  (``a (1 + u) + u |ref| + 2^-133``, ``a = c 2^-24 B`` the fp32 LayerNorm bound, ``u = 2^-8`` for the hi plane, ``2^-16`` for hi + lo);
* every other cache element bit-unchanged, the GARBAGE beyond ``total`` included; idle slots (-1 and >= smax): caches untouched and an
  output head of exact zeros; ``qkv`` bit-unchanged; the output inside a sentinel slab;
* the output against ``R.reference`` evaluated on the planes the kernel wrote (kinds "decode" / "decode_split": the attention tolerance
  is the existing one).  q is never written by the kernel, so it is obtained from a second launch with the q and k column blocks (and
  their LayerNorm parameters) exchanged: the K row that launch appends is the kernel's q, and it is held to the same front bound.
  The planted NaN sits in v: its one output element must be NaN and is left out of the reference (v = 0 there).

The last case runs the same step unfused (clamp_f32_, layernorm_f32_ x 2, attn_decode_rope_rows with identity tables) through the same
checks and compares it with the fused launch bit for bit.
"""
import pytest
import torch

import llama_kernel_ref as R
import mpt_decode_ref as M
from kernel_util import assert_untouched, bits, check_frac, gen, out_slab
from conftest import report_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = R.HD
PAD = 8
CLIP = 0.75
ERR_INVALID, ERR_UNSUPPORTED = -1, -2             # include/llark_hip.h


def _ops():
    from llark_amd import ops
    return ops


class _Case:
    """Inputs of one launch: qkv [batch][ldq] (q, k ~ 1.5 N(0,1), v ~ N(0,1); values planted at +-3 and +-CLIP itself in all three
    blocks, one NaN in v of the first active slot), a history of pos[b] keys per slot (3 for idle slots) with planted keys
    (k_j += 0.6 q: R.decode_plants), GARBAGE beyond it."""

    def __init__(self, nh, batch, pos, smax, split, ln, bias, clip, ldq_pad=8):
        self.nh, self.batch, self.pos, self.smax, self.split, self.clip = nh, batch, list(pos), smax, split, clip
        H = self.H = nh * HD
        g = gen(nh, batch, smax, 5, *[p + 1 for p in pos])
        self.ldq = 3 * H + ldq_pad
        qkv = torch.full((batch, self.ldq), float("nan"))
        qkv[:, :2 * H] = torch.randn(batch, 2 * H, generator=g) * 1.5
        qkv[:, 2 * H:3 * H] = torch.randn(batch, H, generator=g)
        for blk in range(3):
            for i, val in enumerate((3.0, -3.0, CLIP, -CLIP, 40.0)):
                qkv[:, blk * H + 11 + 17 * i + 130 * (i % nh)] = val
        self.live = [b for b in range(batch) if 0 <= pos[b] < smax]
        self.nan_at = (self.live[0], 0, 5)                               # (slot, head, dim) of the NaN in v
        qkv[self.nan_at[0], 2 * H + self.nan_at[1] * HD + self.nan_at[2]] = float("nan")
        self.qkv = qkv
        mk = lambda: torch.randn(H, generator=g)
        self.q_ln = (mk() + 1.0, mk() * 0.5 if bias else None) if ln else None
        self.k_ln = (mk() + 1.0, mk() * 0.5 if bias else None) if ln else None
        self.slopes = R.alibi_slopes(nh)
        self.front = M.front(qkv, nh, clip, self.q_ln, self.k_ln)
        cut = R.planes if split else (lambda x: (x.bfloat16(), None))
        self.hist = [min(p, smax) if p >= 0 else 3 for p in pos]
        kc, vc = [], []
        qref = self.front["q"][0].float().nan_to_num(0.0).view(batch, nh, HD)
        for b in range(batch):
            t = self.hist[b]
            k = torch.randn(nh, t, HD, generator=g) * 1.5
            v = torch.randn(nh, t, HD, generator=g)
            for j in R.decode_plants(t + 1):
                if j < t:
                    k[:, j] += R.PLANT * qref[b]
            kp, vp = cut(k), cut(v)
            kc.append([None if p is None else R.k_cache(p, 1, nh, smax) for p in kp])
            vc.append([None if p is None else R.vt_cache(p, 1, nh, smax) for p in vp])
        np_ = 2 if split else 1
        self.k0 = [torch.cat([kc[b][i] for b in range(batch)]) for i in range(np_)]
        self.vt0 = [torch.cat([vc[b][i] for b in range(batch)]) for i in range(np_)]


def _launch(C, fused, swap, qkv_dev, k, vt, out, out_lo):
    """one decode step on device copies; swap: q and k column blocks (and their LayerNorm parameters) exchanged"""
    ops = _ops()
    H, nh, batch = C.H, C.nh, C.batch
    q_ln, k_ln = (C.k_ln, C.q_ln) if swap else (C.q_ln, C.k_ln)
    if swap:
        qkv_dev = qkv_dev.clone()
        qkv_dev[:, :H], qkv_dev[:, H:2 * H] = qkv_dev[:, H:2 * H].clone(), qkv_dev[:, :H].clone()
    dv = lambda t: None if t is None else t.to(DEV)
    pos = torch.tensor(C.pos, dtype=torch.int32, device=DEV)
    lo = (lambda ps: ps[1]) if C.split else (lambda ps: None)
    sl = C.slopes.to(DEV)
    if fused:
        ops.mpt_attn_decode_rows(qkv_dev[:, :3 * H], batch, nh, HD, pos, C.clip, dv(q_ln and q_ln[0]), dv(q_ln and q_ln[1]), dv(k_ln and k_ln[0]),
                                 dv(k_ln and k_ln[1]), M.LN_EPS, k[0], vt[0], out, lo(k), lo(vt), out_lo, alibi_slopes=sl)
    else:
        x = qkv_dev[:, :3 * H]
        assert x.is_contiguous()
        if C.clip:
            ops.clamp_f32_(x, C.clip)
        if q_ln is not None:
            ops.layernorm_f32_(x[:, :H], dv(q_ln[0]), dv(q_ln[1]), M.LN_EPS)
            ops.layernorm_f32_(x[:, H:2 * H], dv(k_ln[0]), dv(k_ln[1]), M.LN_EPS)
        cos, sin = torch.ones((C.smax, 64), device=DEV), torch.zeros((C.smax, 64), device=DEV)
        ops.attn_decode_rope_rows(x, batch, nh, HD, pos, cos, sin, k[0], vt[0], out, lo(k), lo(vt), out_lo, alibi_slopes=sl)
    torch.cuda.synchronize()
    return qkv_dev


def _check_front(name, C, what, row_planes, b):
    """the planes [nh][128] appended for slot b (K row, V column, or the q of the swapped launch) against the float64 front"""
    ref, a = C.front[what]
    ref = ref[b].view(C.nh, HD)
    nan = torch.isnan(ref)
    got = [p.cpu() for p in row_planes if p is not None]
    for p in got:
        assert bool(torch.isnan(p.float())[nan].all()), f"{name}: the planted NaN is gone"
    if a is None:
        want = R.planes(ref.float()) if C.split else (ref.float().bfloat16(),)
        for i, (p, w) in enumerate(zip(got, want)):
            assert torch.equal(bits(p)[~nan], bits(w)[~nan]), f"{name}: plane {i} is not the clamped value rounded to bf16"
        return
    a = a[b].view(C.nh, HD)
    assert not bool(nan.any())
    report_close(f"{name} hi", got[0].double().numpy(), ref.numpy(), M.plane_tolerance(ref, a, False).numpy())
    if C.split:
        report_close(f"{name} hi+lo", R.value(*got).numpy(), ref.numpy(), M.plane_tolerance(ref, a, True).numpy())


def _run(C, name, fused=True):
    nh, batch, smax, H, split = C.nh, C.batch, C.smax, C.H, C.split
    kind = "decode_split" if split else "decode"
    k, vt = [p.to(DEV, copy=True) for p in C.k0], [p.to(DEV, copy=True) for p in C.vt0]
    slabs = [out_slab(batch * H, torch.bfloat16, front=PAD) for _ in range(2 if split else 1)]
    outs = [s[0].to(DEV, copy=True) for s in slabs]
    view = lambda o: o[PAD:PAD + batch * H].view(batch, H)
    qkv_dev = C.qkv.to(DEV, copy=True)
    after = _launch(C, fused, False, qkv_dev, k, vt, view(outs[0]), view(outs[1]) if split else None)
    if fused:
        assert torch.equal(bits(after), bits(C.qkv)), f"{name}: qkv was written"
    for o, (before, m) in zip(outs, slabs):
        assert_untouched(f"{name} out slab", o, before, m)
    # the swapped launch: its K rows are the kernel's q
    k2, vt2 = [p.to(DEV, copy=True) for p in C.k0], [p.to(DEV, copy=True) for p in C.vt0]
    o2 = [torch.empty((batch, H), dtype=torch.bfloat16, device=DEV) for _ in outs]
    _launch(C, fused, True, C.qkv.to(DEV, copy=True), k2, vt2, o2[0], o2[1] if split else None)
    got = R.value(*[view(o).cpu().view(batch, nh, HD) for o in outs])
    kh, vh, k2h = [p.cpu() for p in k], [p.cpu() for p in vt], [p.cpu() for p in k2]
    for b in range(batch):
        p = C.pos[b]
        wk, wv = torch.zeros(C.k0[0].shape, dtype=torch.bool), torch.zeros(C.vt0[0].shape, dtype=torch.bool)
        if b in C.live:
            wk[b, :, p, :] = True
            wv[b, :, :, p] = True
        for i in range(len(kh)):
            assert_untouched(f"{name} slot {b} K plane {i}", kh[i][b], C.k0[i][b], wk[b])
            assert_untouched(f"{name} slot {b} V^T plane {i}", vh[i][b], C.vt0[i][b], wv[b])
        if b not in C.live:
            assert bool((got[b] == 0).all()), f"{name}: idle slot {b} (position {p}) has a non-zero output"
            continue
        _check_front(f"{name} slot {b} k", C, "k", [x[b, :, p, :] for x in kh], b)
        _check_front(f"{name} slot {b} v", C, "v", [x[b, :, :, p] for x in vh], b)
        qp = [x[b, :, p, :] for x in k2h]
        _check_front(f"{name} slot {b} q", C, "q", qp, b)
        # the attention on the planes the kernel wrote
        kv = R.value(*[x[b, :, :p + 1, :] for x in kh])
        vv = R.value(*[x[b, :, :, :p + 1].transpose(1, 2) for x in vh])
        nan = torch.isnan(vv)
        ref = R.reference(R.value(*qp)[:, None, :], kv, vv.nan_to_num(0.0), p, C.slopes.double())
        skip = nan.any(1)                                           # [nh][128]: output elements fed by the NaN
        assert bool(torch.isnan(got[b])[skip].all()), f"{name} slot {b}: the NaN in v did not reach its output element"
        atol, r = R.out_tolerance(kind, ref)
        keep = ~skip
        check_frac(f"{name} slot {b} pos {p} out", got[b][keep], ref.out[:, 0][keep], atol[:, 0][keep.numpy()], r)
    return dict(k=kh, vt=vh, out=[view(o).cpu() for o in outs])


def _positions(which, smax):
    return [-1, 0, 7, 8] if which == 0 else [255, 256, smax - 1, smax + 3]


VARIANTS = [(ln, bias, clip) for ln, bias in ((False, False), (True, False), (True, True)) for clip in (CLIP, None)]


@pytest.mark.parametrize("ln,bias,clip", VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("which", [0, 1], ids=["pos-1_0_7_8", "pos255_256_last_over"])
@pytest.mark.parametrize("smax", [264, 512])
@pytest.mark.parametrize("nh", [2, 3])
def test_mpt_attn_decode_rows(nh, smax, which, split, ln, bias, clip):
    """16 waves (nh * 4 workgroups): width 256 and 384 (w4 = 96: the LayerNorm lanes are partly idle), positions on both sides of the
    8-key V chunk and of the 256-key round of the K pass, the last position, idle slots"""
    C = _Case(nh, 4, _positions(which, smax), smax, split, ln, bias, clip)
    _run(C, f"mpt_decode nh={nh} smax={smax} {'split' if split else 'bf16'} ln={ln} bias={bias} clip={clip} pos={C.pos}")


@pytest.mark.parametrize("split,ln,bias,clip", [(True, True, True, CLIP), (False, False, False, None), (False, True, False, CLIP)],
                         ids=["split-ln-bias-clip", "bf16-plain", "bf16-ln-clip"])
def test_mpt_attn_decode_rows_four_waves(split, ln, bias, clip):
    """nh * batch = 256 workgroups: the 4-wave form (width 2048, MPT-1B's)"""
    pos = [0, 130, 7, 8, 127, 128, -1, 129, 64, 63, 1, 100, 136, 31, 15, 16]
    C = _Case(16, 16, pos, 136, split, ln, bias, clip)
    _run(C, f"mpt_decode 4 waves {'split' if split else 'bf16'} ln={ln} clip={clip}")


def test_mpt_attn_decode_rows_equals_the_unfused_sequence():
    """clamp_f32_, layernorm_f32_ x 2 and attn_decode_rope_rows with identity tables pass the same checks, and the fused launch
    reproduces their caches and outputs bit for bit (same lane layout and reduction order of the row statistics)"""
    for split in (True, False):
        C = _Case(3, 4, [-1, 8, 255, 0], 264, split, True, True, CLIP, ldq_pad=0)
        fused = _run(C, f"fused {'split' if split else 'bf16'}")
        unfused = _run(C, f"unfused {'split' if split else 'bf16'}", fused=False)
        nan_ok = lambda a, b: torch.equal(bits(a), bits(b)) or bool(((bits(a) == bits(b)) | (torch.isnan(a.float()) & torch.isnan(b.float()))).all())
        for key in ("k", "vt", "out"):
            for i, (a, b) in enumerate(zip(fused[key], unfused[key])):
                assert nan_ok(a, b), f"{key} plane {i}: fused and unfused differ in {int((bits(a) != bits(b)).sum())} elements"


def test_mpt_attn_decode_rows_refusals():
    """each refusal returns an error before any launch (caches, output and qkv bit-unchanged) and names the argument"""
    from llark_amd import _lib
    L = _lib.lib()
    nh, batch, smax = 2, 2, 16
    H = nh * HD
    qkv = torch.randn(batch, 3 * H, device=DEV)
    pos = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    kc, kcl = (R.garbage((batch, nh, smax, HD)).to(DEV) for _ in range(2))
    vc, vcl = (R.garbage((batch, nh, HD, smax)).to(DEV) for _ in range(2))
    out, outl = (R.garbage((batch, H)).to(DEV) for _ in range(2))
    w = torch.ones(64 * HD + HD, device=DEV)
    sl = R.alibi_slopes(nh).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()

    def call(hd=HD, smax_=smax, slopes=sl, lo=(None, None, None), nh_=nh, ldq=3 * H):
        return L.llark_mpt_attn_decode_rows(p(qkv), ldq, batch, nh_, hd, p(pos), 0.75, p(w), None, p(w), None, 1e-5, p(kc), p(vc), p(lo[0]), p(lo[1]),
                                            smax_, p(out), p(lo[2]), p(slopes), st)

    before = [t.clone() for t in (qkv, kc, vc, kcl, vcl, out, outl)]
    for what, rc, kw in (("hd", ERR_UNSUPPORTED, dict(hd=64)), ("smax", ERR_INVALID, dict(smax_=12)), ("alibi_slopes", ERR_INVALID, dict(slopes=None)),
                         ("lo planes", ERR_INVALID, dict(lo=(kcl, None, None))), ("lo planes", ERR_INVALID, dict(lo=(kcl, vcl, None))),
                         ("nh", ERR_UNSUPPORTED, dict(nh_=65, ldq=3 * 65 * HD)), ("ldq", ERR_INVALID, dict(ldq=3 * H - 4)),
                         ("ldq", ERR_INVALID, dict(ldq=3 * H + 2))):
        got = call(**kw)
        msg = L.llark_last_error().decode()
        assert got == rc and msg.startswith("mpt_attn_decode_rows:") and what in msg, (what, got, msg)
    torch.cuda.synchronize()
    for a, b in zip((qkv, kc, vc, kcl, vcl, out, outl), before):
        assert torch.equal(bits(a), bits(b)), "a refused call wrote to a buffer"
