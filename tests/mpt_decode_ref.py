"""Float64 reference and bounds for the front of the MPT ragged decode step (csrc/llama.hip: mpt_attn_decode_kernel), i.e. what happens
to a row of the fused q | k | v product before the attention: clamp to +-clip_qkv (v too; a NaN is kept), the LayerNorm of q_ln / k_ln
over the whole nh*128-wide clamped q row, respectively k row, and one rounding to the bf16 plane(s).  The attention itself is checked
with tests/llama_kernel_ref.py on the planes the kernel wrote.

Bounds (per element; nothing here is taken from the kernel under test):

* no qk_ln: the clamp is exact in fp32, so the planes are ``planes(clamp(x))`` bit for bit.
* qk_ln: the fp32 LayerNorm is within ``a = c 2^-24 B`` of the float64 one, with ``B = rstd |gamma| (|x| + mean|x|) + |beta|`` and
  ``c = max(16, 4 r)``, ``r`` the worst ratio of torch's own float32 CPU layer_norm on the same clamped row -- the bound
  tests/test_mpt_kernels_gpu.py derives for layernorm_f32_ (``kernel_util.tol``).  That fp32 value y (|y| <= |ref| + a) is then rounded:
      one plane      |bf16(y) - ref|   <= a + 2^-8 |y|  + 2^-133 <= a (1 + 2^-8)  + 2^-8 |ref|  + 2^-133
      hi + lo        |hi + lo - ref|   <= a + 2^-16 |y| + 2^-133 <= a (1 + 2^-16) + 2^-16 |ref| + 2^-133
  (hi carries 8 bits and lo 8 more; 2^-133 is bf16's absolute spacing below its normal range, as in ``kernel_util.bf16_ulp``).
"""
import torch

from kernel_util import tol

LN_EPS = 1e-5


def clamp(x, clip):
    """torch.clamp keeps a NaN, in any dtype; clip None / 0: no clamp"""
    return x.clamp(-clip, clip) if clip else x.clone()


def layernorm(x, gamma, beta, eps=LN_EPS):
    """(float64 LayerNorm over the last axis, the fp32 bound a = c 2^-24 B per element as a tensor) of the fp32 rows ``x``"""
    width = x.shape[-1]
    x64, g64 = x.double(), gamma.double()
    b64 = beta.double() if beta is not None else None
    ref = torch.nn.functional.layer_norm(x64, (width,), g64, b64, eps)
    rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + eps)
    bound = rstd * g64.abs() * (x64.abs() + x64.abs().mean(-1, keepdim=True)) + (b64.abs() if b64 is not None else 0.0)
    t32 = torch.nn.functional.layer_norm(x, (width,), gamma, beta, eps)
    atol, _ = tol("qk_ln", t32, ref, bound)
    return ref, torch.from_numpy(atol)


def front(qkv, nh, clip, q_ln=None, k_ln=None, eps=LN_EPS):
    """qkv fp32 [batch][>= 3 nh 128] -> dict name -> (float64 value [batch][nh*128], fp32 bound a or None when the value is exact in
    fp32) for "q", "k", "v".  q_ln / k_ln: (gamma, beta or None) or None."""
    H = nh * 128
    out = {}
    for i, (name, ln) in enumerate((("q", q_ln), ("k", k_ln), ("v", None))):
        x = clamp(qkv[:, i * H:(i + 1) * H].contiguous(), clip)
        if ln is None:
            out[name] = (x.double(), None)
        else:
            out[name] = layernorm(x, ln[0], ln[1], eps)
    return out


def plane_tolerance(ref64, a, two_planes):
    """the bound of the module docstring for bf16(y) (one plane) or hi + lo against the float64 value, as a tensor"""
    u = 2.0 ** -16 if two_planes else 2.0 ** -8
    return a.double() * (1.0 + u) + u * ref64.abs() + 2.0 ** -133
