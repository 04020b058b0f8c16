"""Shared by the kernel-level GPU tests (test_mpt_kernels_gpu.py, test_clap_kernels_gpu.py, test_train_kernels_gpu.py): seeded generators, sentinel
buffers with a bit-exact "nothing else was written" check, and the fp32 tolerance ``c * 2**-24 * B`` whose constant is measured
on torch's own float32 CPU result of the same operation (never on the kernel under test)."""
import torch

from conftest import report_close

EPS24 = 2.0 ** -24
BF_SENTINEL = 0x7FB5            # a bf16 NaN with a recognisable payload


def bf16_ulp(ref64):
    """one bf16 ulp of ``ref64`` (numpy): 2**-8 |ref| for normal values, the format's absolute spacing 2**-133 below 2**-126"""
    return 2.0 ** -8 * ref64.abs().numpy() + 2.0 ** -133


def gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def tol(name, torch32, ref64, bound, under=None):
    """c * 2**-24 * B with c = max(16, 4 * torch's own worst ratio on these inputs).  ``under`` (optional, per element): the absolute
    error fp32 may make where an intermediate falls below its normal range (2**-126 times what multiplies that intermediate); it is
    added to the tolerance and taken off the error before the ratio, so an underflow does not inflate ``c`` for every other element."""
    ref64, bound = ref64.double(), bound.double()
    err = (torch32.double() - ref64).abs()
    if under is not None:
        err = (err - under.double()).clamp_min(0.0)
    pos = bound > 0
    assert bool((err[~pos] == 0).all()), f"{name}: torch fp32 is off where the bound is 0"
    r = float((err[pos] / (EPS24 * bound[pos])).max()) if pos.any() else 0.0
    c = max(16.0, 4.0 * r)
    atol = c * EPS24 * bound
    return (atol if under is None else atol + under.double()).numpy(), r


def check(name, got, ref64, atol, rtol=0.0, bound=None, r_torch=None, under=None):
    got64 = got.detach().cpu().double()
    if bound is not None:
        pos = bound > 0
        err = (got64 - ref64).abs() if under is None else ((got64 - ref64).abs() - under.double()).clamp_min(0.0)
        k = float((err[pos] / (EPS24 * bound.double()[pos])).max()) if pos.any() else 0.0
        print(f"[ratio] {name}: kernel {k:.3g} x 2^-24 B, torch fp32 {r_torch:.3g}")
    return report_close(name, got64.numpy(), ref64.numpy(), atol, rtol)


def bits(t):
    return t.detach().cpu().contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def nan_buf(rows, ld):
    return torch.full((rows, ld), float("nan"), dtype=torch.float32)


def bf_sentinel(shape):
    return torch.full(shape, BF_SENTINEL, dtype=torch.int16).view(torch.bfloat16)


F16_SENTINEL = 0x7DB5           # an fp16 NaN with a recognisable payload
U8_SENTINEL = 0xA5


def f16_sentinel(shape):
    return torch.full(shape, F16_SENTINEL, dtype=torch.int16).view(torch.float16)


def u8_sentinel(shape):
    return torch.full(shape, U8_SENTINEL, dtype=torch.uint8)


def assert_untouched(name, after, before, written):
    """every element outside the boolean mask ``written`` is bit-identical to what it was before the launch"""
    a, b = bits(after), bits(before)
    keep = ~written
    assert torch.equal(a[keep], b[keep]), f"{name}: {int((a[keep] != b[keep]).sum())} elements outside the output were written"


def mask(shape, rows, c0, c1):
    m = torch.zeros(shape, dtype=torch.bool)
    m[:rows, c0:c1] = True
    return m


def slab(x, front=3, back=4):
    """``x`` (fp32 / bf16, any shape) flattened into a 1-D sentinel buffer at element offset ``front`` (odd by default: how the trainers
    slice their flat buffers): returns (buffer, boolean mask of the elements that belong to x)"""
    n = x.numel()
    buf = bf_sentinel((front + n + back,)) if x.dtype == torch.bfloat16 else torch.full((front + n + back,), float("nan"), dtype=x.dtype)
    buf[front:front + n] = x.reshape(-1)
    m = torch.zeros(front + n + back, dtype=torch.bool)
    m[front:front + n] = True
    return buf, m


def out_slab(n, dtype, front=3, back=4):
    """an all-sentinel 1-D buffer whose elements [front, front + n) are an output: (buffer, boolean mask of the output)"""
    size = front + n + back
    buf = bf_sentinel((size,)) if dtype == torch.bfloat16 else torch.full((size,), float("nan"), dtype=dtype)
    m = torch.zeros(size, dtype=torch.bool)
    m[front:front + n] = True
    return buf, m


def check_frac(name, got, ref64, atol, r_torch):
    """``check`` for outputs whose tolerance ``atol`` (numpy, per element) is a format term plus ``c * 2**-24 * B``: prints the kernel's
    worst error as a fraction of that tolerance next to torch's float32 ratio ``r`` that set ``c``"""
    got64 = got.detach().cpu().double()
    err = (got64 - ref64.double()).abs().numpy()
    pos = atol > 0
    k = float((err[pos] / atol[pos]).max()) if pos.any() else 0.0
    print(f"[ratio] {name}: kernel {k:.3g} of its tolerance, torch fp32 {r_torch:.3g} x 2^-24 B")
    return report_close(name, got64.numpy(), ref64.double().numpy(), atol)
