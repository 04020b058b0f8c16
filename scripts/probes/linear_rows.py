"""Are the decode Linears row-count independent in bits?  Row 0 of an m-row ops.gemm16 call against the 1-row call at the 7B decode
shapes, both flows, row 0 of the 5 / 8 / 16-row calls against each other, and the RMSNorm-fused one-row form against the unfused and the 8-row forms.  Prints one line per case
(profiles/linear_rows_probe.txt); run from the repository root: `python scripts/probes/linear_rows.py`."""
import sys, os, json
sys.path.insert(0, os.getcwd())
import torch
from llark_amd import ops
dev = "cuda"
g = torch.Generator().manual_seed(0)
bf = torch.bfloat16
res = []
for name, K, N, epi in (("qkv", 4096, 12288, "F32"), ("o", 4096, 4096, "RESID"), ("down", 11008, 4096, "RESID"), ("lm_head", 4096, 32003, "F32")):
    w = (torch.randn(N, K, generator=g) * 0.02).to(bf).to(dev)
    x = torch.randn(16, K, generator=g)
    for split in (False, True):
        hi = x.to(bf).to(dev)
        lo = (x - x.to(bf).float()).to(bf).to(dev) if split else None
        outs = {}
        for m in (1, 2, 4, 5, 8, 16):
            c = torch.zeros(m, N, dtype=torch.float32, device=dev)
            r = torch.ones(m, N, dtype=torch.float32, device=dev) if epi == "RESID" else None
            ops.gemm16(hi[:m].contiguous(), None if lo is None else lo[:m].contiguous(), w, None, N, getattr(ops, "EPI_" + epi), c=c, resid=r)
            torch.cuda.synchronize()
            outs[m] = c[0].clone()
        eq = {m: bool(torch.equal(outs[m].view(torch.int32), outs[1].view(torch.int32))) for m in outs}
        same = lambda a, b: bool(torch.equal(outs[a].view(torch.int32), outs[b].view(torch.int32)))
        res.append({"linear": name, "split": split, "row0_equals_m1": eq, "row0_m5_m8_m16_equal": same(5, 8) and same(8, 16),
                    "row0_m2_equals_m4": same(2, 4)})
        print(res[-1], flush=True)
# RMSNorm inside the GEMM (m = 1 form) against rmsnorm_bf16 + gemm16
K, N = 4096, 12288
w = (torch.randn(N, K, generator=g) * 0.02).to(bf).to(dev)
nw = (1 + 0.1 * torch.randn(K, generator=g)).to(dev)
h = torch.randn(8, K, generator=g).to(dev)
for split in (False, True):
    c1 = torch.zeros(1, N, dtype=torch.float32, device=dev)
    ops.gemm16_rmsnorm_a(h[:1].contiguous(), nw, 1e-5, w, N, ops.EPI_F32, split, c=c1)
    x16 = torch.empty(8, K, dtype=bf, device=dev); x16l = torch.empty_like(x16) if split else None
    ops.rmsnorm_bf16(h, nw, 1e-5, x16, x16l)
    c8 = torch.zeros(8, N, dtype=torch.float32, device=dev)
    ops.gemm16(x16, x16l, w, None, N, ops.EPI_F32, c=c8)
    c8a = torch.zeros(8, N, dtype=torch.float32, device=dev)
    ops.gemm16_rmsnorm_a(h, nw, 1e-5, w, N, ops.EPI_F32, split, c=c8a)
    torch.cuda.synchronize()
    print({"rmsnorm_a m1 vs rmsnorm+gemm16 m8 row0": bool(torch.equal(c1[0].view(torch.int32), c8[0].view(torch.int32))),
           "rmsnorm_a m1 vs rmsnorm_a m8 row0": bool(torch.equal(c1[0].view(torch.int32), c8a[0].view(torch.int32))), "split": split}, flush=True)
