"""Ragged MPT training step at MPT-1B dimensions (d_model 2048, 16 heads, 24 blocks, expansion 4; random weights): the existing loop --
one right-padded ``HipMptTrainer.forward_backward`` per micro-batch -- against ``--pack_sequences`` -- the whole optimizer step as ONE
packed stream on the ALiBi variable-length attention kernels -- in ONE process on one GPU, the two modes alternating step by step on
the SAME trainer after warm-up (the MPT sibling of scripts/bench_train_packed.py).

    python scripts/bench_mpt_train_packed.py [--steps 5] [--warmup 2] [--layers 24] [--out profiles/mpt_train_packed.json]

8 examples per optimizer step (micro-batch 2 x accumulation 4) with the lengths of the README's "Ragged data" measurement
(663, 500, 603, 614, 403, 403, 374, 536): a CLAP-style prompt (<audio_start>, one 512-d frame, <audio_end>, 128 prompt tokens) plus a
response.  Per mode: ms per optimizer step (median and every sample), rows processed per step, and -- from one more step of each with an
event pair around every timed launch -- the time of the variable-length attention calls summed over the blocks."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llark_amd import ops  # noqa: E402
from llark_amd.m2t.data import pack_sequences  # noqa: E402
from llark_amd.m2t.mpt_engine import HipMptEngine, MptDims  # noqa: E402
from llark_amd.m2t.mpt_train_engine import HipMptTrainer  # noqa: E402

PAD_ID = 0
V = 50432 + 3
START, END, PATCH = V - 2, V - 1, V - 3
PROMPT = 4 + 128


def examples(lengths, device, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for ln in lengths:
        ids = torch.tensor([0, START, PATCH, END] + torch.randint(3, 50000, (ln - 4,), generator=gen).tolist())
        labels = ids.clone()
        labels[:PROMPT] = -100
        out.append((ids, labels, torch.randn(1, 512, generator=gen).to(device)))
    return out


def build(args, device, s_total: int, max_len: int):
    dims = MptDims(vocab_size=V, mm_hidden_size=512, n_layers=args.layers)
    # two cache slots hold the longest micro-batch of the loop AND the packed stream: no cache is reallocated when the modes alternate
    eng = HipMptEngine(dims, device, max_batch=args.micro, max_seq=ops.round_up(max(max_len, -(-s_total // args.micro)), 64), precision="bf16")
    g = torch.Generator(device=device).manual_seed(0)
    D, E = dims.d_model, dims.expansion_ratio * dims.d_model

    def n(*shape):
        return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * 0.02).to(torch.bfloat16)

    ones = lambda: torch.ones(D, device=device)
    sd = {"transformer.wte.weight": n(V, D), "transformer.norm_f.weight": ones(), "transformer.mm_projector.weight": n(D, 512),
          "transformer.mm_projector.bias": torch.zeros(D, device=device)}
    for i in range(dims.n_layers):
        p = f"transformer.blocks.{i}"
        sd.update({f"{p}.norm_1.weight": ones(), f"{p}.norm_2.weight": ones(), f"{p}.attn.Wqkv.weight": n(3 * D, D),
                   f"{p}.attn.out_proj.weight": n(D, D), f"{p}.ffn.up_proj.weight": n(E, D), f"{p}.ffn.down_proj.weight": n(D, E)})
    eng.load_state_dict(sd)
    return eng, HipMptTrainer(eng, lr=5e-5)


def loop_step(tr, micro_batches, accum):
    for ids, labels, segs in micro_batches:
        tr.forward_backward(ids, segs, labels, 1.0 / accum)
    tr.step(1, max_grad_norm=1.0)


def packed_step(tr, plan):
    tr.forward_backward_packed(plan=plan)
    tr.step(1, max_grad_norm=1.0)


def measure(args, device) -> dict:
    lengths = [int(x) for x in args.lengths.split(",")]
    assert len(lengths) == args.micro * args.accum, "lengths must number micro x accum"
    ex = examples(lengths, device, args.seed)
    plan = pack_sequences([e[0] for e in ex], [e[1] for e in ex], [args.micro] * args.accum, [(b, 1, e[2]) for b, e in enumerate(ex)], PAD_ID)
    micro_batches = []
    for k in range(args.accum):
        grp = ex[k * args.micro: (k + 1) * args.micro]
        S = max(int(e[0].numel()) for e in grp)
        ids = torch.full((args.micro, S), PAD_ID, dtype=torch.long)
        labels = torch.full((args.micro, S), -100, dtype=torch.long)
        for b, e in enumerate(grp):
            ids[b, : e[0].numel()], labels[b, : e[0].numel()] = e[0], e[1]
        micro_batches.append((ids.to(device), labels.to(device), [(b, 1, e[2]) for b, e in enumerate(grp)]))
    eng, tr = build(args, device, plan.s_total, max(lengths))
    for _ in range(args.warmup):
        loop_step(tr, micro_batches, args.accum)
        packed_step(tr, plan)
    torch.cuda.synchronize()
    ms = {"loop": [], "packed": []}
    for _ in range(args.steps):                          # the two modes alternate: what else runs on the box hits both alike
        for mode in ("loop", "packed"):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            loop_step(tr, micro_batches, args.accum) if mode == "loop" else packed_step(tr, plan)
            t1.record()
            torch.cuda.synchronize()
            ms[mode].append(t0.elapsed_time(t1))
    kernel_ms = {}
    for mode in ("loop", "packed"):                      # one more step of each with an event pair around every timed launch
        ops.start_kernel_timing()
        loop_step(tr, micro_batches, args.accum) if mode == "loop" else packed_step(tr, plan)
        timers = ops.stop_kernel_timing()
        kernel_ms[mode] = {k: {"launches": v[0], "ms": round(v[1], 3)} for k, v in sorted(timers.items(), key=lambda kv: -kv[1][1])}
    med = statistics.median
    out = {"lengths": lengths, "tokens_per_step": sum(lengths),
           "loop": {"ms_per_step": round(med(ms["loop"]), 2), "ms_per_step_all": [round(x, 2) for x in ms["loop"]],
                    "rows_per_step": sum(int(m[0].numel()) for m in micro_batches), "weight_passes": args.accum, "kernel_ms": kernel_ms["loop"]},
           "packed": {"ms_per_step": round(med(ms["packed"]), 2), "ms_per_step_all": [round(x, 2) for x in ms["packed"]],
                      "rows_per_step": plan.s_total, "weight_passes": 1, "kernel_ms": kernel_ms["packed"]}}
    out["packed_over_loop"] = round(out["packed"]["ms_per_step"] / out["loop"]["ms_per_step"], 4)
    out["attention_varlen_ms"] = {k: v for k, v in kernel_ms["packed"].items() if k.startswith("attn_")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--micro", type=int, default=2)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--lengths", default="663,500,603,614,403,403,374,536")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join("profiles", "mpt_train_packed.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    res = {"shape": {"backbone": "mpt-1b", "d_model": 2048, "n_heads": 16, "layers": args.layers, "expansion_ratio": 4, "micro_batch": args.micro,
                     "accumulation": args.accum, "seed": args.seed}, "device": torch.cuda.get_device_name(0)}
    res["full"] = measure(args, device)
    print(json.dumps({m: {k: v for k, v in res["full"][m].items() if k != "kernel_ms"} for m in ("loop", "packed")}),
          json.dumps(res["full"]["attention_varlen_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
