"""Training step at 7B dimensions (random weights, the recipe shape: micro-batches of 2 x 2048, accumulation 4) in the three recipes
of ``HipLlamaTrainer``, one after the other in ONE process on one GPU: LoRA (r = 64 on all seven projections), frozen backbone, and
full fine-tuning -- the baseline the other two are read against (same box, same process, the unchanged default code path).

    python scripts/bench_lora_train.py [--steps 3] [--warmup 1] [--layers 32] [--modes lora,lora_separate,frozen,full]
                                       [--out profiles/lora_train.json]

``lora`` carries the adapters in extra K columns of the operand twins (fused RoPE / SwiGLU epilogues kept); ``lora_separate`` is the same
recipe with every adapter as separate low-rank products around the base products (LLARK_TRAIN_LORA_AUG=0), measured beside it.

Per mode: ms per optimizer step (median), forward / backward ms of a micro-batch, ms of the optimizer part (clip + AdamW + operand
refresh), peak allocated HBM, and -- from one extra step with per-kernel HIP events -- ``kernel_ms`` per kernel family
(``lora_down`` / ``lora_dw`` are the new launches; the adapters' up-projections run under ``gemm_bf16``)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llark_amd import ops  # noqa: E402
from llark_amd.m2t.bench_support import END, FRAMES, START, VOCAB, make_prompt_ids  # noqa: E402
from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims  # noqa: E402
from llark_amd.m2t.lora import LoraConfig  # noqa: E402
from llark_amd.m2t.train_engine import HipLlamaTrainer  # noqa: E402


def build(mode: str, args, device):
    dims = LlamaDims(vocab_size=VOCAB)
    dims.num_hidden_layers = args.layers
    eng = HipLlamaEngine(dims, device, max_batch=args.micro, max_seq=ops.round_up(args.seq, 64), precision="bf16")
    g = torch.Generator(device=device).manual_seed(0)
    H, I = dims.hidden_size, dims.intermediate_size

    def n(*shape):
        return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * 0.02).to(torch.bfloat16)

    ones = torch.ones(H, device=device)
    for i in range(dims.num_hidden_layers):
        eng.set_layer(i, n(H, H), n(H, H), n(H, H), n(H, H), n(I, H), n(I, H), n(H, I), ones, ones)
    eng.set_globals(n(VOCAB, H), ones, n(VOCAB, H), n(H, dims.mm_hidden_size), torch.zeros(H, device=device))
    kw = {}
    if mode in ("lora", "lora_separate"):
        kw["lora"] = LoraConfig(r=args.lora_r, alpha=16)
    elif mode == "frozen":
        kw["freeze_backbone"] = True
    os.environ["LLARK_TRAIN_LORA_AUG"] = "0" if mode == "lora_separate" else "1"
    tr = HipLlamaTrainer(eng, lr=5e-5, embed_grad_tokens=[START, END], **kw)
    del os.environ["LLARK_TRAIN_LORA_AUG"]
    if "lora" in kw:                                   # non-zero B: at the zero initialisation dA is identically zero
        for name, p in tr.params:
            if name.endswith(".lora_B"):
                p[:, : args.lora_r].normal_(0.0, 0.01, generator=g)
        tr._refresh_lora()
    tr.time_phases = True
    gen = torch.Generator().manual_seed(11)
    batches = []
    for k in range(args.accum):
        ids = make_prompt_ids(args.micro, seed=100 + k)
        ans = torch.randint(3, 32000, (args.micro, args.seq - ids.shape[1]), generator=gen)
        full = torch.cat([ids, ans], dim=1)
        labels = full.clone()
        labels[:, : ids.shape[1]] = -100
        emb = torch.randn(args.micro, FRAMES, dims.mm_hidden_size, generator=gen)
        batches.append((full.to(device), labels.to(device), emb.to(device)))
    return eng, tr, batches


def one_step(tr, batches, accum):
    """(forward ms, backward ms) events of the last micro-batch; the optimizer step follows."""
    for k, (ids, labels, emb) in enumerate(batches):
        segs = [(b, 1, emb[b]) for b in range(ids.shape[0])]
        tr.forward_backward(ids, segs, labels, 1.0 / accum, last_micro_batch=k == len(batches) - 1)
    ev = tr.phase_events
    opt0, opt1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    opt0.record()
    tr.step(1, max_grad_norm=1.0)
    opt1.record()
    return ev, (opt0, opt1)


def measure(mode: str, args, device) -> dict:
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    eng, tr, batches = build(mode, args, device)
    static = torch.cuda.memory_allocated()
    for _ in range(args.warmup):
        one_step(tr, batches, args.accum)
    torch.cuda.synchronize()
    step_ms, fwd_ms, bwd_ms, opt_ms = [], [], [], []
    for _ in range(args.steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ev, opt = one_step(tr, batches, args.accum)
        t1.record()
        torch.cuda.synchronize()
        step_ms.append(t0.elapsed_time(t1))
        fwd_ms.append(ev[0].elapsed_time(ev[1]))
        bwd_ms.append(ev[1].elapsed_time(ev[2]))
        opt_ms.append(opt[0].elapsed_time(opt[1]))
    peak = torch.cuda.max_memory_allocated()
    ops.start_kernel_timing()                            # one more step with an event pair around every timed launch
    one_step(tr, batches, args.accum)
    timers = ops.stop_kernel_timing()
    med = statistics.median
    out = {"ms_per_step": round(med(step_ms), 2), "ms_per_step_all": [round(x, 2) for x in step_ms],
           "micro_batch_forward_ms": round(med(fwd_ms), 2), "micro_batch_backward_ms": round(med(bwd_ms), 2),
           "optimizer_ms": round(med(opt_ms), 2), "peak_allocated_gb": round(peak / 1e9, 2), "static_allocated_gb": round(static / 1e9, 2),
           "trainable_elements": int(tr.flat_grad.numel()),
           "kernel_ms": {k: {"launches": v[0], "ms": round(v[1], 2)} for k, v in sorted(timers.items(), key=lambda kv: -kv[1][1])}}
    del eng, tr, batches
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--micro", type=int, default=2)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--lora_r", type=int, default=64)
    ap.add_argument("--modes", default="lora,lora_separate,frozen,full")
    ap.add_argument("--out", default=os.path.join("profiles", "lora_train.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    res = {"shape": {"layers": args.layers, "micro_batch": args.micro, "seq": args.seq, "accumulation": args.accum, "lora_r": args.lora_r},
           "device": torch.cuda.get_device_name(0)}
    for mode in args.modes.split(","):
        res[mode] = measure(mode, args, device)
        print(mode, json.dumps({k: v for k, v in res[mode].items() if k != "kernel_ms"}), flush=True)
    if "full" in res:
        for mode in ("lora", "lora_separate", "frozen"):
            if mode in res:
                res[mode]["step_time_vs_full"] = round(res[mode]["ms_per_step"] / res["full"]["ms_per_step"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
