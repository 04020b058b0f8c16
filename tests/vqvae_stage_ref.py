"""References, emulation, planted defects and the tolerance for the kernel-level tests of the fused VQ-VAE stage kernel
(csrc/vqvae_fused.hip: vq_stage_kernel<CIN, OUTCONV, NTW>, 12 instantiations behind llark_vqvae_stage_f16x2).  A plain module:
tests/test_vqvae_stage_kernels_gpu.py runs the kernel against it, tests/test_vqvae_stage_ref_cpu.py proves on the CPU that its
tolerance rejects wrong kernels and accepts the documented arithmetic.  torch only; nothing outside the repository is read.

One stage:  Conv1d(cin -> 32, k 4, s 2, p 1);  depth x [ x + W2 . relu(W1 (*)_d relu(x) + b1) + b2 ];  optionally
Conv1d(32 -> 64, k 3, p 1) on the RAW block output.  Every layer pads with ZEROS at both clip ends.

``stage_ref64``   the dense float64 evaluation on the exact operands: float64(hi) + float64(lo) of the input planes (or the fp32
                  audio) and the fp32 weights as float64.
``stage_emulate`` the documented arithmetic: weights as fp16 hi / lo planes of W 2^e (e = ops.vqvae_weight_exponent), activations
                  split to fp16 hi / lo where the kernel splits them (relu(x) in front of each dilated conv, the hidden activation in
                  front of the 1x1, the raw block output in front of the output conv), three passes Wh.xh, Wh.xl, Wl.xh per k-step of
                  16 channels accumulated in fp32 in the kernel's k-step order (tap-major; b 2^e first, 2^-e on the way out; the
                  residual enters the 1x1's accumulator as (x + b2) 2^e), the cin = 1 convolution as the fp32 fmaf chain (bias, taps
                  ascending).  The 16 products of one MFMA are summed in float64 and rounded to fp32 once: one legal order of the
                  hardware's sum, whose own order is not documented.
``defects_for``   planted defects: variants of ``stage_emulate(defect=...)`` a checker must reject, those a configuration can express.

The tolerance.  A propagated worst-case bound is useless here: absolute-weight propagation through four blocks gives ~2e2 where the
emulation is ~1e-6 off at max|y| ~ 7.6.  So it is MEASURED -- on the emulation, never on the kernel -- per case and output tensor:

    tol = MARGIN * max|stage_emulate - stage_ref64| + 2^-24 max|stage_ref64|,          MARGIN = 4

MARGIN covers what is not documented (the order of the sum inside an MFMA and the fused rounding between steps); the second term is
half an ulp of the fp32 the result is delivered in.  tests/test_vqvae_stage_ref_cpu.py requires every planted defect to miss the
reference by >= 8 tol, so the margin cannot hide one.

Measured.  The emulation sits at 0.23-0.25 of tol by construction (1 / MARGIN, less the 2^-24 term); max|emulation - ref64| is
1.9e-6 at max|y| = 7.2 for (cin 32, dilations 1 3 9 27, output conv), i.e. 2.6e-7 relative.

  * planted defects, CPU (tests/test_vqvae_stage_ref_cpu.py; max|defect - ref64| / tol, both output tensors): the smallest over the
    three configurations is 72.4 -- the Wh.xl pass dropped in the 1x1 of block 0, (cin 32, 1 3 9 27, output conv); the dropped passes
    are the closest calls (72-130 x tol, wherever they are dropped), the halo one position short is 2.6e3, every other defect is
    above 1e3 (b1 not scaled by 2^e: 2e4-7e4).  MARGIN could be 8 and the smallest ratio would still be 36 >= 2 * 8.
  * kernel error / tol on an MI355X (tests/test_vqvae_stage_kernels_gpu.py, 89 cases x {fp32, planes}; 16-tile window), smallest and
    largest per instantiation:

        cin  1, no output conv   0.191 .. 0.411          cin  1, output conv   0.180 .. 0.407
        cin 32, no output conv   0.227 .. 0.462          cin 32, output conv   0.250 .. 0.445
        cin 64, no output conv   0.214 .. 0.407          cin 64, output conv   0.180 .. 0.380

    the 32-tile window (bit-equal to the 16-tile one on 256 clips of t = 1857; four clips against float64): 0.27 .. 0.35.
    weights x 1e-3 / x 30, inputs with subnormal lo planes and silence lie in the same range (0.21 .. 0.33).  The kernel is where
    the emulation is, within the factor of two that the undocumented summation order may take: no case is above 0.5, nothing had to
    be changed in the kernel's arithmetic.  What the tests did change is the launcher: a dilation above the 32 guard rows of the LDS
    window (accepted before whenever the sum fitted the 48-position halo, e.g. (1, 6, 36) or depth 1 with dilation 48) is refused.
"""
import re
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
MARGIN = 4.0
EPS24 = 2.0 ** -24
TT16 = 416                       # output positions of the 16-tile window (512 - 2 * 48); the 32-tile window holds 928
TT32 = 928
HALO = 48


# --------------------------------------------------------------------------------------------------------------------
# the launcher's rules, restated from the constants of the source (parsed: a change there shows up here)
# --------------------------------------------------------------------------------------------------------------------
def launcher_constants():
    src = (ROOT / "llark_amd" / "csrc" / "vqvae_fused.hip").read_text()
    c = {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("VF_HALO", "VF_MAXDEPTH", "VF_GUARD")}
    assert re.search(r"constexpr int GUARD = VF_GUARD;", src), "the kernel's guard rows are no longer tied to VF_GUARD"
    assert re.search(r"dil\[i\] > VF_GUARD", src), "the launcher's dilation rule is no longer tied to VF_GUARD"
    return c


def launcher_refusal(n, cin, tin, dils, out_conv):
    """None where llark_vqvae_stage_f16x2 takes the shape, else a word its llark_last_error message must contain (the argument it
    names).  Order of the checks as in the launcher."""
    c = launcher_constants()
    if n <= 0 or tin < 2 or tin % 2:
        return "tin"
    if cin not in (1, 32, 64):
        return "cin"
    if not 1 <= len(dils) <= c["VF_MAXDEPTH"]:
        return "depth"
    rf = 1 if out_conv else 0
    for d in dils:
        if d < 1 or d > c["VF_GUARD"]:
            return "dilation"
        rf += d
    if rf > c["VF_HALO"]:
        return "receptive field"
    return None


def window_tiles(n, t):
    """tiles per window the launcher picks: 32 (928 outputs) from n t >= 512 * 928 on, else 16 (416 outputs)"""
    return 32 if n * t >= 512 * TT32 else 16


# --------------------------------------------------------------------------------------------------------------------
# weights and inputs
# --------------------------------------------------------------------------------------------------------------------
def make_weights(cin, dils, out_conv, amp_w=1.0, seed=0):
    """plain fp32 weights of one stage: standard deviation amp_w / sqrt(fan_in) (activations stay O(1) over four blocks at
    amp_w = 1), biases 0.1 min(amp_w, 1)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * cin + 31 * sum((i + 1) * d for i, d in enumerate(dils)) + int(out_conv))

    def rn(*shape, fan=None):
        s = amp_w / fan ** 0.5 if fan else 0.1 * min(amp_w, 1.0)
        return (torch.randn(*shape, generator=g) * s).float()

    w = dict(cin=cin, dil=list(dils), amp=amp_w, w0=rn(32, cin, 4, fan=4 * cin), b0=rn(32), w1=[], b1=[], w2=[], b2=[], wo=None, bo=None)
    for _ in dils:
        w["w1"].append(rn(32, 32, 3, fan=96))
        w["b1"].append(rn(32))
        w["w2"].append(rn(32, 32, 1, fan=32))
        w["b2"].append(rn(32))
    if out_conv:
        w["wo"], w["bo"] = rn(64, 32, 3, fan=96), rn(64)
    return w


def build_stage(cin, dils, out_conv, amp_w=1.0, seed=0, device="cuda"):
    """the ``st`` dict ops.vqvae_stage takes (packed by ops.vqvae_pack_frag16 on the device, like VQVAE._make_stage) with the plain
    fp32 weights under st["ref"]"""
    from llark_amd import ops

    w = make_weights(cin, dils, out_conv, amp_w, seed)
    dev = torch.device(device)

    def d(x):
        return x.to(dev).contiguous()

    st = dict(cin=cin, b0=d(w["b0"]), w0f=None, w0_hi=None, w0_lo=None, wo_hi=None, wo_lo=None, bo=None, dil=list(dils), ref=w)
    wexp = [0]
    if cin == 1:
        st["w0f"] = ops.pack_conv_weight(d(w["w0"]))
    else:
        wexp[0] = ops.vqvae_weight_exponent(w["w0"])
        st["w0_hi"], st["w0_lo"] = ops.vqvae_pack_frag16(d(w["w0"]), exp2=wexp[0])
    hi, lo, br = [], [], []
    for i in range(len(dils)):
        e3, e1 = ops.vqvae_weight_exponent(w["w1"][i]), ops.vqvae_weight_exponent(w["w2"][i])
        h3, l3 = ops.vqvae_pack_frag16(d(w["w1"][i]), exp2=e3)
        h1, l1 = ops.vqvae_pack_frag16(d(w["w2"][i]), perm1x1=True, exp2=e1)
        hi += [h3, h1]
        lo += [l3, l1]
        br += [d(w["b1"][i]), d(w["b2"][i])]
        wexp += [e3, e1]
    st["wr_hi"], st["wr_lo"], st["br"] = torch.cat(hi).contiguous(), torch.cat(lo).contiguous(), torch.cat(br).contiguous()
    wexp.append(0)
    if out_conv:
        wexp[-1] = ops.vqvae_weight_exponent(w["wo"])
        st["wo_hi"], st["wo_lo"] = ops.vqvae_pack_frag16(d(w["wo"]), exp2=wexp[-1])
        st["bo"] = d(w["bo"])
    st["wexp"] = wexp
    return st


def split16(v32):
    """fp32 -> fp16 planes hi = fp16(v), lo = fp16(v - hi) (round to nearest even, subnormals kept): the kernel's split2"""
    v32 = v32.float()
    hi = v32.half()
    return hi, (v32 - hi.float()).half()


def make_input(cin, n, tin, seed, scale=1.0, zero=False):
    """cin == 1: audio fp32 [n][tin]; else fp16 planes (hi, lo) [n][tin][cin] of a gaussian of standard deviation ``scale``"""
    g = torch.Generator().manual_seed(77 * seed + 13 * tin + n + 1000 * cin)
    v = torch.zeros(n, tin, cin) if zero else torch.randn(n, tin, cin, generator=g) * scale
    return v[:, :, 0].contiguous() if cin == 1 else split16(v)


def operand64(x):
    """the exact operand [n][cin][tin] float64 the kernel is given"""
    if isinstance(x, (tuple, list)):
        return (x[0].double() + x[1].double()).permute(0, 2, 1).contiguous()
    return x.double()[:, None, :]


# --------------------------------------------------------------------------------------------------------------------
# float64 reference
# --------------------------------------------------------------------------------------------------------------------
def stage_ref64(x, w):
    """dense float64 evaluation -> [n][C][tin / 2]"""
    y = F.conv1d(operand64(x), w["w0"].double(), w["b0"].double(), stride=2, padding=1)
    for i, d in enumerate(w["dil"]):
        h = F.conv1d(F.relu(y), w["w1"][i].double(), w["b1"][i].double(), dilation=d, padding=d)
        y = y + F.conv1d(F.relu(h), w["w2"][i].double(), w["b2"][i].double())
    if w["wo"] is not None:
        y = F.conv1d(y, w["wo"].double(), w["bo"].double(), padding=1)
    return y


# --------------------------------------------------------------------------------------------------------------------
# emulation of the documented arithmetic
# --------------------------------------------------------------------------------------------------------------------
# a planted defect is a tuple: (kind, argument ...)
#   ("drop", "lh" | "hl", layer)   the Wl.xh / Wh.xl pass is missing in ONE layer: "w0", ("c3", i), ("1x1", i) or "wo"
#   ("nomask", "left" | "right")   positions outside the clip keep their computed value between layers at that clip end
#   ("halo", 47)                   windowed evaluation whose halo is one position short of a receptive field of 48
#   ("relu_out",)  ("relu_in",)    a ReLU in front of the output conv / the strided conv
#   ("perm1x1", i)                 the 1x1 weights of block i in plain channel order against accumulator-register order activations
#   ("b1_unscaled", i)  ("b2_dropped", i)  ("taps_reversed", i)
#   ("phase",)                     strided conv reads 2 t + tap instead of 2 t - 1 + tap
#   ("halves",)                    the two 32-channel halves of the output conv's weights swapped
def _wplanes(w32):
    from llark_amd import ops

    e = ops.vqvae_weight_exponent(w32)
    hi, lo = split16(w32 * 2.0 ** e)
    return hi.double(), lo.double(), 2.0 ** e, 2.0 ** -e


def _mfma(acc, a, b):
    """acc fp32 [n][co][L] + a [co][16] . b [n][16][L] (float64 values of fp16 operands): one v_mfma_f32_32x32x16_f16"""
    return (acc.double() + torch.matmul(a, b)).float()


def _shift(x, sh):
    """x[..., i + sh] with zeros outside the evaluated range: the zero guard rows of the LDS window"""
    if sh == 0:
        return x
    L = x.shape[-1]
    if abs(sh) >= L:
        return torch.zeros_like(x)
    return F.pad(x[..., sh:], (0, sh)) if sh > 0 else F.pad(x[..., :L + sh], (-sh, 0))


def _conv(acc, wh, wl, fetch, drop):
    """tap-major k-steps of 16 channels, three passes each"""
    _, cin, k = wh.shape
    for tap in range(k):
        for c0 in range(0, cin, 16):
            xh, xl = fetch(tap, c0)
            a, b = wh[:, c0:c0 + 16, tap], wl[:, c0:c0 + 16, tap]
            acc = _mfma(acc, a, xh)
            if drop != "hl":
                acc = _mfma(acc, a, xl)
            if drop != "lh":
                acc = _mfma(acc, b, xh)
    return acc


def _emulate_range(x, w, lo, hi, defect):
    """fp32 [n][C][hi - lo]: the stage at positions lo .. hi - 1 of the stage-rate axis, everything outside that range read as zero
    (= one workgroup's window with its guard rows); the residual stream stays unmasked, what the next layer reads is masked"""
    kind = defect[0] if defect else None
    cin, dils = w["cin"], w["dil"]
    t = (x[0].shape[1] if cin > 1 else x.shape[1]) // 2
    tin = 2 * t
    pos = torch.arange(lo, hi)
    inclip = (pos >= 0) & (pos < t)
    keep = inclip.clone()
    if kind == "nomask":
        keep |= (pos < 0) if defect[1] == "left" else (pos >= t)

    def drop_at(layer):
        return defect[1] if kind == "drop" and defect[2] == layer else None

    def gather(src, tap):                       # src [n][c][tin] -> [n][c][L] at input index 2 pos - 1 + tap, zero outside the clip
        idx = 2 * pos - 1 + tap + (1 if kind == "phase" else 0)
        ok = (idx >= 0) & (idx < tin)
        return src[:, :, idx.clamp(0, tin - 1)] * ok

    def store(v, relu):                         # store_tiles: (relu,) mask, split
        v = F.relu(v) if relu else v
        h, l = split16(v * keep)
        return h.double(), l.double()

    # the strided convolution
    if cin == 1:
        a = x.float()[:, None, :]
        a = F.relu(a) if kind == "relu_in" else a
        acc = w["b0"].float()[None, :, None].expand(a.shape[0], 32, len(pos)).contiguous()
        for tap in range(4):                    # fmaf(w, x, s): the product is exact in float64, one rounding to fp32
            acc = (w["w0"][:, 0, tap].double()[None, :, None] * gather(a, tap).double() + acc.double()).float()
    else:
        xh, xl = x[0].float().permute(0, 2, 1), x[1].float().permute(0, 2, 1)
        if kind == "relu_in":
            xh, xl = split16(F.relu(xh + xl))
            xh, xl = xh.float(), xl.float()
        wh, wl, m, im = _wplanes(w["w0"])
        acc = (w["b0"].float() * m)[None, :, None].expand(xh.shape[0], 32, len(pos)).contiguous()
        acc = _conv(acc, wh, wl, lambda tap, c0: (gather(xh[:, c0:c0 + 16], tap).double(), gather(xl[:, c0:c0 + 16], tap).double()),
                    drop_at("w0")) * im
    sh_, sl_ = store(acc, True)

    for i, d in enumerate(dils):
        w1h, w1l, m1, i1 = _wplanes(w["w1"][i])
        w2 = w["w2"][i]
        if kind == "perm1x1" and defect[1] == i:
            # the kernel's k index 8 g + j of k-step s holds hidden channel 16 s + (j & 3) + 8 (j >> 2) + 4 g; a weight packed in
            # plain order has column 16 s + 8 g + j there
            bad = torch.empty_like(w2)
            for s in range(2):
                for g in range(2):
                    for j in range(8):
                        bad[:, 16 * s + (j & 3) + 8 * (j >> 2) + 4 * g] = w2[:, 16 * s + 8 * g + j]
            w2 = bad
        w2h, w2l, m2, i2 = _wplanes(w2)
        sign = -1 if kind == "taps_reversed" and defect[1] == i else 1
        b1 = w["b1"][i].float() * (1.0 if kind == "b1_unscaled" and defect[1] == i else m1)
        ha = b1[None, :, None].expand_as(acc).contiguous()
        ha = _conv(ha, w1h, w1l, lambda tap, c0: (_shift(sh_[:, c0:c0 + 16], sign * (tap - 1) * d), _shift(sl_[:, c0:c0 + 16], sign * (tap - 1) * d)),
                   drop_at(("c3", i)))
        hh, hl = split16(F.relu(ha) * i1)
        hh, hl = hh.double(), hl.double()
        b2 = torch.zeros(32) if kind == "b2_dropped" and defect[1] == i else w["b2"][i].float()
        acc = (acc + b2[None, :, None]) * m2
        acc = _conv(acc, w2h, w2l, lambda tap, c0: (hh[:, c0:c0 + 16], hl[:, c0:c0 + 16]), drop_at(("1x1", i))) * i2
        if i + 1 < len(dils):
            sh_, sl_ = store(acc, True)
        elif w["wo"] is not None:
            sh_, sl_ = store(acc, kind == "relu_out")

    if w["wo"] is None:
        return acc
    wo = torch.cat([w["wo"][32:], w["wo"][:32]]) if kind == "halves" else w["wo"]
    woh, wol, mo, io = _wplanes(wo)
    oa = (w["bo"].float() * mo)[None, :, None].expand(acc.shape[0], 64, len(pos)).contiguous()
    return _conv(oa, woh, wol, lambda tap, c0: (_shift(sh_[:, c0:c0 + 16], tap - 1), _shift(sl_[:, c0:c0 + 16], tap - 1)), drop_at("wo")) * io


def stage_emulate(x, w, defect=None, halo=None, tt=TT16):
    """fp32 [n][C][t].  halo=None: dense (one range over the clip; with a "nomask" defect HALO positions beyond it on both sides);
    halo=h: windows of ``tt`` outputs evaluated with h extra positions either side, as the kernel's workgroups do"""
    t = (x[0].shape[1] if w["cin"] > 1 else x.shape[1]) // 2
    if defect and defect[0] == "halo":
        halo = defect[1]
    if halo is None:
        ext = HALO if defect and defect[0] == "nomask" else 0
        return _emulate_range(x, w, -ext, t + ext, defect)[:, :, ext:ext + t].contiguous()
    out = [_emulate_range(x, w, t0 - halo, t0 + tt + halo, defect)[:, :, halo:halo + min(tt, t - t0)] for t0 in range(0, t, tt)]
    return torch.cat(out, dim=2).contiguous()


def planes_value(v32):
    """what the (hi, lo) output planes of an fp32 result hold, as float64"""
    h, l = split16(v32)
    return h.double() + l.double()


def tolerance(emu, ref64, margin=MARGIN):
    return margin * float((emu.double() - ref64).abs().max()) + EPS24 * float(ref64.abs().max())


def defects_for(w, t):
    """the planted defects the configuration can express"""
    last = len(w["dil"]) - 1
    out = [("drop", "lh", ("c3", 0)), ("drop", "hl", ("c3", 0)), ("drop", "lh", ("1x1", last)), ("drop", "hl", ("1x1", last)),
           ("drop", "lh", ("c3", last)), ("drop", "hl", ("1x1", 0)),
           ("nomask", "left"), ("nomask", "right"), ("relu_in",), ("perm1x1", 0), ("perm1x1", last), ("b1_unscaled", last), ("b2_dropped", 0),
           ("taps_reversed", last), ("phase",)]
    if w["cin"] > 1:
        out += [("drop", "lh", "w0"), ("drop", "hl", "w0")]
    if w["wo"] is not None:
        out += [("drop", "lh", "wo"), ("drop", "hl", "wo"), ("relu_out",), ("halves",)]
    if sum(w["dil"]) + (w["wo"] is not None) == HALO and t > TT16:
        out.append(("halo", HALO - 1))
    return out
