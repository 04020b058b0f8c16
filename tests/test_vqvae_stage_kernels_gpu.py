"""GPU: the fused VQ-VAE stage kernel (csrc/vqvae_fused.hip, llark_vqvae_stage_f16x2: 3 cin x output conv or not x 2 window
geometries) against the dense float64 reference of tests/vqvae_stage_ref.py, at the shapes the launcher accepts and the
end-to-end tests never run: depth 1-4, dilations up to the 32 guard rows, receptive fields 46 and 48 (= the halo), t odd, t < 32 and
t on either side of a tile or window edge, every output combination.  The tolerance is measured on the CPU emulation of the
documented arithmetic (never on the kernel): see the module docstring of vqvae_stage_ref.py, which also records what was measured."""
import pytest
import torch

import kernel_util as U
import vqvae_stage_ref as R
from conftest import report_close

pytestmark = pytest.mark.gpu

TS = (1, 31, 32, 33, 367, 368, 369, 415, 416, 417, 464, 465, 833)
DILS = ((1,), (27,), (32,), (1, 3), (1, 3, 9, 27), (1, 3, 9, 32), (2, 4, 9, 32))
INST = ((1, False), (1, True), (32, False), (32, True), (64, False), (64, True))
F_FRONT, F_BACK, H_SLACK = 3, 4, 64              # fp32 buffers start at an odd element; fp16 planes keep their 16-byte alignment


def _cases():
    out = []
    for ii, (cin, oc) in enumerate(INST):                   # every instantiation meets every t; dilation sets and n rotate
        for ti, t in enumerate(TS):
            out.append(dict(cin=cin, oc=oc, t=t, dils=DILS[(ti + 2 * ii) % 7], n=(1, 3)[(ti + ii) % 2]))
    for cin in (1, 32, 64):                                 # receptive field 48 across a window edge, 46 next to it
        out.append(dict(cin=cin, oc=True, t=833, dils=(2, 4, 9, 32), n=1))
    out.append(dict(cin=32, oc=True, t=417, dils=(1, 3, 9, 32), n=3))
    # the exponent range of wexp: weights 1e-3 and 30 x the unit scale (inputs scaled so that the fp16 planes do not overflow)
    out.append(dict(cin=32, oc=True, t=369, dils=(1, 3, 9, 27), n=1, amp=1e-3))
    out.append(dict(cin=1, oc=False, t=417, dils=(1,), n=1, amp=30.0, scale=0.05))
    out.append(dict(cin=64, oc=True, t=33, dils=(1,), n=3, amp=30.0, scale=0.01))
    # activations mostly below 2^-3: subnormal lo planes
    out.append(dict(cin=32, oc=True, t=465, dils=(1, 3, 9, 27), n=1, scale=2.0 ** -7))
    out.append(dict(cin=1, oc=False, t=368, dils=(1, 3), n=3, scale=2.0 ** -7))
    # silence
    out.append(dict(cin=1, oc=True, t=417, dils=(1, 3, 9, 27), n=1, zero=True))
    out.append(dict(cin=32, oc=False, t=33, dils=(27,), n=3, zero=True))
    return out


def _id(c):
    s = f"cin{c['cin']}-oc{int(c['oc'])}-t{c['t']}-n{c['n']}-d{'_'.join(map(str, c['dils']))}"
    for k in ("amp", "scale"):
        if k in c:
            s += f"-{k}{c[k]:g}"
    return s + ("-zero" if c.get("zero") else "")


CASES = _cases()
_stages = {}
_ratios = {}


def _stage(cin, dils, oc, amp=1.0):
    key = (cin, tuple(dils), oc, amp)
    if key not in _stages:
        _stages[key] = R.build_stage(cin, dils, oc, amp, seed=11)
    return _stages[key]


def _to_device(x):
    """the input on the device inside sentinel slack (NaN): a read outside [0, n tin cin) would poison the result"""
    def one(v, front, back, sentinel):
        buf = sentinel((front + v.numel() + back,))
        buf[front:front + v.numel()] = v.reshape(-1)
        return buf.cuda()[front:front + v.numel()]
    if isinstance(x, tuple):
        return tuple(one(p, H_SLACK, H_SLACK, U.f16_sentinel) for p in x)
    return one(x, F_FRONT, F_BACK, lambda s: torch.full(s, float("nan")))


def _launch(st, xd, n, tin, mode):
    """mode: "f32", "planes" or "both" -> (f32 [n][C][t] or None, (hi, lo) [n][t][C] or None), CPU; the slack around every output
    buffer is checked bit for bit"""
    from llark_amd import ops
    t, c = tin // 2, 64 if st["wo_hi"] is not None else 32
    num = n * t * c
    f0 = torch.full((F_FRONT + num + F_BACK,), float("nan"))
    h0 = U.f16_sentinel((H_SLACK + num + H_SLACK,))
    fd = f0.cuda() if mode != "planes" else None
    hd, ld = (h0.cuda(), h0.cuda()) if mode != "f32" else (None, None)
    ops.vqvae_stage(xd, n, st["cin"], tin, st, out_planes=None if hd is None else (hd[H_SLACK:H_SLACK + num], ld[H_SLACK:H_SLACK + num]),
                    out_f32=None if fd is None else fd[F_FRONT:F_FRONT + num])
    torch.cuda.synchronize()
    f = p = None
    if fd is not None:
        m = torch.zeros(f0.numel(), dtype=torch.bool)
        m[F_FRONT:F_FRONT + num] = True
        U.assert_untouched(f"{mode}: out_f32", fd, f0, m)
        f = fd.cpu()[F_FRONT:F_FRONT + num].view(n, c, t)
    if hd is not None:
        m = torch.zeros(h0.numel(), dtype=torch.bool)
        m[H_SLACK:H_SLACK + num] = True
        U.assert_untouched(f"{mode}: out_hi", hd, h0, m)
        U.assert_untouched(f"{mode}: out_lo", ld, h0, m)
        p = (hd.cpu()[H_SLACK:H_SLACK + num].view(n, t, c), ld.cpu()[H_SLACK:H_SLACK + num].view(n, t, c))
    return f, p


def _planes64(p):
    return (p[0].double() + p[1].double()).permute(0, 2, 1)


def _check_outputs(name, st, x, n, tin, key=None):
    """all three output combinations against float64 under the emulation's tolerance; returns the fp32 result"""
    w = st["ref"]
    ref, emu = R.stage_ref64(x, w), R.stage_emulate(x, w)
    xd = _to_device(x)
    f, _ = _launch(st, xd, n, tin, "f32")
    _, p = _launch(st, xd, n, tin, "planes")
    fb, pb = _launch(st, xd, n, tin, "both")
    assert torch.equal(U.bits(fb), U.bits(f)) and torch.equal(U.bits(pb[0]), U.bits(p[0])) and torch.equal(U.bits(pb[1]), U.bits(p[1])), \
        f"{name}: an output depends on which other output was requested"
    hi, lo = R.split16(fb.permute(0, 2, 1))
    assert torch.equal(U.bits(pb[0]), U.bits(hi)) and torch.equal(U.bits(pb[1]), U.bits(lo)), f"{name}: planes are not the fp16 hi / lo split of the fp32 output"
    for what, got, base in (("fp32", f.double(), emu.double()), ("planes", _planes64(p), R.planes_value(emu))):
        tol = R.tolerance(base, ref)
        ratio = float((got - ref).abs().max()) / tol
        emu_ratio = float((base - ref).abs().max()) / tol
        print(f"[stage] {name} {what}: kernel error / tol {ratio:.3f} (emulation {emu_ratio:.3f}), tol {tol:.3e}, max|ref| {float(ref.abs().max()):.3g}")
        if key is not None:
            lo_, hi_ = _ratios.get(key, (ratio, ratio))
            _ratios[key] = (min(lo_, ratio), max(hi_, ratio))
        report_close(f"{name} {what}", got.numpy(), ref.numpy(), tol)
    return f


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_stage_against_float64(c):
    cin, oc, t, n = c["cin"], c["oc"], c["t"], c["n"]
    assert R.launcher_refusal(n, cin, 2 * t, c["dils"], oc) is None and R.window_tiles(n, t) == 16
    st = _stage(cin, c["dils"], oc, c.get("amp", 1.0))
    x = R.make_input(cin, n, 2 * t, seed=t + n, scale=c.get("scale", 1.0), zero=c.get("zero", False))
    print()
    _check_outputs(_id(c), st, x, n, 2 * t, key=(cin, oc))


def test_every_instantiation_met_every_t_class_and_dilation_set():
    for cin, oc in INST:
        mine = [c for c in CASES if (c["cin"], c["oc"]) == (cin, oc)]
        assert {c["t"] for c in mine} >= set(TS) and {c["dils"] for c in mine} >= set(DILS) and {c["n"] for c in mine} == {1, 3}
    assert 80 <= len(CASES) <= 120
    for key in sorted(_ratios):
        print(f"\n[stage] cin {key[0]:2d} output conv {int(key[1])}: kernel error / tol in [{_ratios[key][0]:.3f}, {_ratios[key][1]:.3f}]", end="")


@pytest.mark.parametrize("cin,oc,dils", [(1, False, (1, 3, 9, 27)), (32, True, (3, 32)), (64, False, (32,))], ids=lambda v: str(v))
def test_32_tile_window_equals_16_tile_window_bit_for_bit(cin, oc, dils):
    """n t >= 512 * 928 switches the launcher to the 32-tile window (NTW = 4).  Every position's arithmetic is the same chain in both
    geometries: 256 clips of t = 1857 (windows of 928, 928, 1 outputs) in one launch equal two launches of 128 clips (16-tile windows:
    416, .., 193) bit for bit, fp32 and planes; four clips are checked against float64 through a small launch."""
    from llark_amd import ops
    n, t = 256, 1857
    tin, c = 2 * t, 64 if oc else 32
    assert R.window_tiles(n, t) == 32 and R.window_tiles(n // 2, t) == 16
    st = _stage(cin, dils, oc)
    g = torch.Generator(device="cuda").manual_seed(17 + cin)
    v = torch.randn(n, tin, cin, device="cuda", generator=g)
    if cin == 1:
        x = v[:, :, 0].contiguous()
        part = lambda a, b: x[a:b]
    else:
        hi = v.half()
        x = (hi, (v - hi.float()).half())
        part = lambda a, b: (x[0][a:b], x[1][a:b])
    del v
    num = n * t * c

    def outs():
        return (torch.full((F_FRONT + num + F_BACK,), float("nan"), device="cuda"), U.f16_sentinel((1,)).cuda().repeat(H_SLACK + num + H_SLACK),
                U.f16_sentinel((1,)).cuda().repeat(H_SLACK + num + H_SLACK))

    def call(xs, nn, bufs, clip0):
        o = clip0 * t * c
        ops.vqvae_stage(xs, nn, cin, tin, st, out_planes=(bufs[1][H_SLACK + o:H_SLACK + o + nn * t * c], bufs[2][H_SLACK + o:H_SLACK + o + nn * t * c]),
                        out_f32=bufs[0][F_FRONT + o:F_FRONT + o + nn * t * c])

    big, small = outs(), outs()
    call(x, n, big, 0)
    call(part(0, 128), 128, small, 0)
    call(part(128, 256), 128, small, 128)
    torch.cuda.synchronize()
    assert torch.equal(big[0].view(torch.int32), small[0].view(torch.int32)), "fp32 output differs between the window geometries (or slack was written)"
    assert torch.equal(big[1].view(torch.int16), small[1].view(torch.int16)) and torch.equal(big[2].view(torch.int16), small[2].view(torch.int16))
    for b in big:                                      # the slack is still sentinel, the output is not
        s = b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)
        front = F_FRONT if b.dtype == torch.float32 else H_SLACK
        assert bool((s[:front] == s[0]).all()) and bool((s[front + num:] == s[0]).all()) and not bool(torch.isnan(b[front:front + num]).any())
    clips = [0, 127, 128, 255]
    xs = tuple(p[clips].cpu() for p in x) if cin > 1 else x[clips].cpu()
    print()
    f4 = _check_outputs(f"ntw4 cin{cin} oc{int(oc)} clips {clips}", st, xs, 4, tin)
    got = big[0][F_FRONT:F_FRONT + num].view(n, c, t)[clips].cpu()
    assert torch.equal(U.bits(got), U.bits(f4)), "a clip of the 256-clip launch differs from the same clip in a launch of 4"


@pytest.mark.parametrize("cin,oc,dils", [(1, True, (1, 3, 9, 27)), (32, False, (2, 4, 9, 32)), (64, True, (27,))], ids=lambda v: str(v))
def test_a_clip_does_not_depend_on_its_batch(cin, oc, dils):
    t, st = 417, _stage(cin, dils, oc)
    x = R.make_input(cin, 3, 2 * t, seed=9)
    fb, pb = _launch(st, _to_device(x), 3, 2 * t, "both")
    for i in range(3):
        xi = tuple(p[i:i + 1].contiguous() for p in x) if cin > 1 else x[i:i + 1].contiguous()
        f, p = _launch(st, _to_device(xi), 1, 2 * t, "both")
        assert torch.equal(U.bits(f[0]), U.bits(fb[i])) and torch.equal(U.bits(p[0][0]), U.bits(pb[0][i])) and torch.equal(U.bits(p[1][0]), U.bits(pb[1][i]))


def test_launcher_refuses_what_the_kernel_is_not_built_for():
    """before any launch, llark_last_error naming the argument; a dilation above the 32 guard rows is never launched"""
    from llark_amd import _lib, ops
    st = _stage(32, (1,), False)
    e = st["wexp"][1]
    n, tin = 1, 64
    xd = _to_device(R.make_input(32, n, tin + 2, seed=1))
    num = n * (tin // 2) * 64
    f0 = torch.full((num,), float("nan"))

    def refused(cin, tin_, dils, code=-1):
        word = R.launcher_refusal(n, cin, tin_, dils, False)
        assert word is not None
        bad = dict(st, dil=list(dils), wexp=[st["wexp"][0]] + [e, e] * len(dils) + [0])
        fd = f0.cuda()
        with pytest.raises(_lib.LlarkHipError, match=word) as ei:
            ops.vqvae_stage(xd, n, cin, tin_, bad, out_f32=fd)
        assert f"(code {code})" in str(ei.value), str(ei.value)
        torch.cuda.synchronize()
        assert torch.equal(U.bits(fd), U.bits(f0)), "a refused call wrote its output"

    refused(32, tin + 1, (1,))                             # tin odd
    refused(16, tin, (1,))                                 # cin not built
    refused(32, tin, ())                                   # depth 0
    refused(32, tin, (1, 1, 1, 1, 1))                      # depth 5
    refused(32, tin, (16, 32, 1))                          # receptive field 49
    for dils in ((33,), (48,), (1, 6, 36)):                # sums within the halo, one dilation beyond the guard rows
        refused(32, tin, dils, code=-2)
    fd = f0.cuda()
    ops.vqvae_stage(xd, n, 32, tin, st, out_f32=fd)       # and the unchanged arguments are taken
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fd[:n * (tin // 2) * 32]).all())
