"""CPU: the checker of tests/test_vqvae_stage_kernels_gpu.py (tests/vqvae_stage_ref.py) accepts the documented arithmetic of the fused
VQ-VAE stage kernel and rejects every planted defect by a wide margin -- so the measured tolerance cannot hide a wrong kernel."""
import pytest
import torch

import vqvae_stage_ref as R

# (cin, dilations, output conv, n, t): t = 465 puts a second 16-tile window of 49 positions behind the first, receptive field 48
CONFIGS = [(32, (1, 3, 9, 27), True, 2, 150), (1, (1,), False, 2, 97), (64, (2, 4, 9, 32), True, 1, 465)]
_cache = {}


def _case(cfg):
    if cfg not in _cache:
        cin, dils, oc, n, t = cfg
        w = R.make_weights(cin, dils, oc, 1.0, seed=3)
        x = R.make_input(cin, n, 2 * t, seed=5)
        ref = R.stage_ref64(x, w)
        emu = R.stage_emulate(x, w)
        _cache[cfg] = (w, x, ref, emu)
    return _cache[cfg]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"cin{c[0]}-d{'_'.join(map(str, c[1]))}-oc{int(c[2])}")
def test_emulation_is_fp32_class_and_within_a_quarter_of_its_tolerance(cfg):
    w, x, ref, emu = _case(cfg)
    assert emu.dtype == torch.float32 and emu.shape == ref.shape == (cfg[3], 64 if cfg[2] else 32, cfg[4])
    for name, got in (("fp32", emu.double()), ("planes", R.planes_value(emu))):
        err, tol = float((got - ref).abs().max()), R.tolerance(got, ref)
        print(f"\n[stage emu] {cfg[:3]} {name}: max|emu - ref64| {err:.3e}, max|ref| {float(ref.abs().max()):.3f}, tol {tol:.3e}")
        assert err <= tol / R.MARGIN
        # the emulation is fp32-class: far below the 2^-12 of a single dropped low pass (else the tolerance would be meaningless)
        assert err <= 2.0 ** -18 * float(ref.abs().max())


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"cin{c[0]}-d{'_'.join(map(str, c[1]))}-oc{int(c[2])}")
def test_every_planted_defect_is_rejected_at_8_tol(cfg):
    """... by far: the ratios are printed and the smallest is in the module docstring of vqvae_stage_ref.py (it would still hold at
    twice the margin)"""
    w, x, ref, emu = _case(cfg)
    defects = R.defects_for(w, cfg[4])
    if cfg[0] == 64:
        assert ("halo", 47) in defects
    worst = None
    for d in defects:
        bad = R.stage_emulate(x, w, defect=d)
        for name, got, base in (("fp32", bad.double(), emu.double()), ("planes", R.planes_value(bad), R.planes_value(emu))):
            tol = R.tolerance(base, ref)
            ratio = float((got - ref).abs().max()) / tol
            print(f"[stage defect] {cfg[:3]} {d} {name}: {ratio:.3g} x tol")
            worst = ratio if worst is None else min(worst, ratio)
            assert ratio >= 8.0, f"{d} ({name}) is only {ratio:.3g} x tol away from the reference: the checker would accept it"
    print(f"[stage defect] {cfg[:3]}: smallest ratio {worst:.3g}")


@pytest.mark.parametrize("cin,oc,t", [(64, True, 465), (1, True, 833), (32, True, 417)])
def test_windowed_evaluation_with_halo_48_is_the_dense_one_bit_for_bit(cin, oc, t):
    """receptive field exactly 48 = the halo: what a workgroup computes on its window (zero guard rows beyond it) equals the dense
    evaluation at every output position; one position less and it does not"""
    w = R.make_weights(cin, (2, 4, 9, 32), oc, 1.0, seed=4)
    x = R.make_input(cin, 2, 2 * t, seed=6)
    dense = R.stage_emulate(x, w)
    assert torch.equal(R.stage_emulate(x, w, halo=48).view(torch.int32), dense.view(torch.int32))
    short = R.stage_emulate(x, w, halo=47)
    differs = sorted(set((short != dense).nonzero()[:, 2].tolist()))           # only a window's outermost output reaches that far
    edges = [p for k in range(1, t // R.TT16 + 1) for p in (k * R.TT16 - 1, k * R.TT16) if p < t]
    assert differs and set(differs) <= set(edges), (differs, edges)
    # ... and the 32-tile geometry (928 outputs per window) is the same chain per position
    if t > 500:
        assert torch.equal(R.stage_emulate(x, w, halo=48, tt=R.TT32), dense) is True


def test_launcher_rule_helper():
    c = R.launcher_constants()
    assert c == dict(VF_HALO=48, VF_MAXDEPTH=4, VF_GUARD=32)
    ok = R.launcher_refusal
    assert ok(1, 1, 2, (1,), False) is None and ok(3, 64, 1666, (2, 4, 9, 32), True) is None and ok(1, 32, 64, (32,), False) is None
    assert ok(1, 32, 64, (1, 3, 9, 27), True) is None and ok(1, 32, 64, (16, 32), False) is None
    assert ok(1, 32, 833, (1,), False) == "tin" and ok(1, 32, 0, (1,), False) == "tin"
    assert ok(1, 16, 64, (1,), False) == "cin"
    assert ok(1, 32, 64, (), False) == "depth" and ok(1, 32, 64, (1, 1, 1, 1, 1), False) == "depth"
    assert ok(1, 32, 64, (2, 4, 9, 32), True) is None and ok(1, 32, 64, (2, 4, 10, 32), True) == "receptive field"
    assert ok(1, 32, 64, (16, 32, 1), False) == "receptive field"
    # the rule that was missing: sums within the halo whose single dilation leaves the 32 guard rows of the LDS window
    assert ok(1, 32, 64, (1, 6, 36), False) == "dilation" and ok(1, 32, 64, (48,), False) == "dilation" and ok(1, 32, 64, (33,), False) == "dilation"
    assert ok(1, 32, 64, (0,), False) == "dilation"
    assert R.window_tiles(256, 1857) == 32 and R.window_tiles(128, 1857) == 16 and R.window_tiles(3, 833) == 16
