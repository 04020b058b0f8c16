"""Instruction-tuning loop with the hyper-parameters of the reference's ``m2t/train.py`` +
``scripts/training/train_llark.sh:20-49`` on the native HIP training step (``HipLlamaTrainer``, or ``HipMptTrainer`` when the model
name contains "mpt": m2t/train.py:62, scripts/training/train_mpt_model.sh): per-device
micro-batches, gradient accumulation, AdamW (lr 5e-5, weight decay 0), cosine schedule with 3 % linear warm-up,
data-parallel gradient all-reduce over RCCL, bf16.

Three recipes of the reference run here: full fine-tuning (the default), ``--freeze_backbone True`` (adapter-only pre-training,
m2t/train.py:79,146-148) and ``--lora_enable True`` (m2t/train.py:82-99: rank-r adapters on q/k/v/o/gate/up/down_proj over a frozen
base; ``llark_amd/m2t/lora.py``).  The MPT backbone runs the first of the three (its script sets none of the other flags; they are
refused by name), with ``wte`` frozen as the reference leaves it (m2t/models/mpt.py:405-411).

Not reproduced (I/O + HF-Trainer glue out of scope): webdataset / GCS readers, wandb logging,
HF ``TrainingArguments`` parsing, LoRA dropout / bias training, bitsandbytes / FSDP options.  Batches are the dictionaries produced by
``llark_amd.m2t.prompting.DataCollatorForSupervisedDataset`` (same keys as the reference's collator).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Iterable, Optional

import torch

from .. import dist as D
from .llamav2 import plan_audio_splice
from .train_engine import HipLlamaTrainer


@dataclass
class TrainConfig:
    learning_rate: float = 5e-5                 # train_llark.sh:26
    weight_decay: float = 0.0                   # :37
    warmup_ratio: float = 0.03                  # :36
    max_steps: int = 100000                     # :38
    gradient_accumulation_steps: int = 4        # :27
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    lr_scheduler_type: str = "cosine"           # :35
    gradient_checkpointing: bool = False        # train_llark.sh:25 (per-layer recompute in the backward; same gradients, less HBM)
    max_grad_norm: float = 1.0                  # transformers TrainingArguments default (clip_grad_norm_ in Trainer's step); not set by train_llark.sh
    fuse_accumulation: bool = False             # run the accumulation micro-batches of a step as ONE pass when they share a shape and the engine
                                                # holds them (loss normalised per micro-batch: the same gradient; 8 x 2048: 714 -> 685 ms, +60 GB)
    pack_sequences: bool = False                # run the step's ragged micro-batches as ONE packed stream: no pad rows, one pass over the weights
                                                # (variable-length attention; loss normalised per micro-batch: the same gradient)
    grad_comm: str = "bf16"                     # the reference's DDP buckets are bf16 (m2t/train.py:94-103 casts the model): 13.5 GB/step; "fp32" = 27 GB
    freeze_backbone: bool = False               # m2t/train.py:79,146-148: only mm_projector and the audio-token embedding rows train
    lora_enable: bool = False                   # m2t/train.py:82-99 (implies a frozen base)
    lora_r: int = 64
    lora_alpha: float = 16.0
    lora_dropout: float = 0.0                   # the reference's default is 0.05; dropout is not built
    lora_bias: str = "none"
    seed: int = 42                              # adapter initialisation


def lora_config_of(cfg) -> "Optional[LoraConfig]":
    """The LoraConfig of a TrainConfig / parsed argument namespace (None when ``lora_enable`` is off)."""
    from .lora import LoraConfig

    if not getattr(cfg, "lora_enable", False):
        return None
    return LoraConfig(r=int(cfg.lora_r), alpha=float(cfg.lora_alpha), dropout=float(cfg.lora_dropout), bias=str(cfg.lora_bias))


def lr_at(step: int, cfg: TrainConfig) -> float:
    """HF ``get_cosine_schedule_with_warmup`` (step counted from 0)."""
    warm = math.ceil(cfg.max_steps * cfg.warmup_ratio)
    if step < warm:
        return cfg.learning_rate * step / max(1, warm)
    prog = (step - warm) / max(1, cfg.max_steps - warm)
    return cfg.learning_rate * max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))


MPT_UNSUPPORTED = {"freeze_backbone": "adapter-only pre-training", "lora_enable": "LoRA adapters",
                   "gradient_checkpointing": "per-block recompute in the backward"}


def backbone_of(model_name_or_path: str) -> str:
    """The reference's rule (m2t/train.py:62): a model name that contains "mpt" selects ``WrappedMPTForCausalLM``, anything else
    ``WrappedLlamav2ForCausalLM``."""
    return "mpt" if "mpt" in str(model_name_or_path) else "llama"


def check_mpt_recipe(args) -> None:
    """The recipes the MPT training step does not implement, refused by flag name (``args``: a TrainConfig or a parsed namespace)."""
    for flag, what in MPT_UNSUPPORTED.items():
        if getattr(args, flag, False):
            raise NotImplementedError(f"--{flag} True: {what} is not implemented for the MPT training step (HipMptTrainer trains the whole "
                                      "backbone; scripts/training/train_mpt_model.sh does not set this flag)")


def train(engine, batches: Iterable[Dict], audio_cfg, cfg: TrainConfig = TrainConfig(), world: int = 1,
          max_optimizer_steps: Optional[int] = None, log=None, output_dir: Optional[str] = None, save_steps: int = 5000,
          save_total_limit: Optional[int] = 1, rank: int = 0, hf_config=None, tokenizer=None):
    """engine: a bf16 ``HipLlamaEngine`` or ``HipMptEngine`` holding the weights; batches: collated micro-batches of THIS rank
    (``input_ids``, ``labels``, ``attention_mask``, ``audio_encodings``).  Returns the list of logged losses.
    With ``output_dir``: resumes from the newest ``checkpoint-*`` there (m2t/train.py:257-260), saves every
    ``save_steps`` optimizer steps (train_llark.sh:31,41-42) and once more at the end; ``hf_config`` / ``tokenizer`` are
    written into every checkpoint folder so that ``from_pretrained`` / ``load_pretrained_model`` can open it.
    ``batches`` may be a callable ``skip_micro_batches -> iterable``: it is then called with the number of micro-batches
    the resumed run has already consumed (``step * gradient_accumulation_steps``) so the data stream continues."""
    from .engine import HipLlamaEngine
    from .mpt_engine import HipMptEngine

    mpt = isinstance(engine, HipMptEngine)
    if cfg.pack_sequences and not mpt and not isinstance(engine, HipLlamaEngine):
        raise NotImplementedError(f"--pack_sequences: packing is built for the training steps of HipLlamaEngine and HipMptEngine, not for "
                                  f"{type(engine).__name__}")
    comm = torch.bfloat16 if cfg.grad_comm == "bf16" else torch.float32
    if mpt:
        from .mpt_train_engine import HipMptTrainer

        check_mpt_recipe(cfg)
        tr = HipMptTrainer(engine, lr=cfg.learning_rate, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                           weight_decay=cfg.weight_decay, train_wte=False, grad_comm=comm)
        # the keyword differences of the two trainers: the MPT step has no per-layer all-reduce start and no norm collection of its own
        # (allreduce_grads / step do both in one pass afterwards)
        forward_backward = lambda ids, segs, labels, scale, **kw: tr.forward_backward(ids, segs, labels, scale)
        forward_backward_packed = lambda plan, **kw: tr.forward_backward_packed(plan=plan)
    else:
        toks = [t for t in (audio_cfg.audio_start_token, audio_cfg.audio_end_token) if isinstance(t, int)]
        tr = HipLlamaTrainer(engine, lr=cfg.learning_rate, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                             weight_decay=cfg.weight_decay, embed_grad_tokens=toks, grad_comm=comm,
                             gradient_checkpointing=cfg.gradient_checkpointing, freeze_backbone=cfg.freeze_backbone,
                             lora=lora_config_of(cfg), lora_seed=cfg.seed)
        forward_backward = tr.forward_backward
        forward_backward_packed = lambda plan, **kw: tr.forward_backward_packed(None, None, None, None, plan=plan, **kw)
    fuse = cfg.fuse_accumulation and not mpt
    if cfg.fuse_accumulation and mpt and cfg.gradient_accumulation_steps > 1:
        note = "--fuse_accumulation: the MPT training step has no fused accumulation; running the per-micro-batch loop (same gradient)"
        if log:
            log(dict(note=note))
        else:
            import logging

            logging.getLogger(__name__).warning(note)
    from . import checkpoint as CK

    if output_dir:
        CK.maybe_resume(tr, output_dir)
    if callable(batches):
        batches = batches(tr.step_count * cfg.gradient_accumulation_steps)
    if max_optimizer_steps and tr.step_count >= max_optimizer_steps:
        return []
    losses, acc, micro = [], 0.0, 0
    accum = cfg.gradient_accumulation_steps
    pending = []                                            # fuse_accumulation: the step's micro-batches until the last one arrives

    def run_micro(ids, segs, labels, last):
        loss = forward_backward(ids, segs, labels, 1.0 / accum, overlap_allreduce_world=world if last else 1,
                                last_micro_batch=last and cfg.max_grad_norm > 0)
        return float(loss.item()) / accum

    pad_id = getattr(tokenizer, "pad_token_id", None)
    pad_id = 0 if pad_id is None else int(pad_id)

    def end_of_step() -> bool:
        """exchange, optimizer step, log, checkpoint; True when ``max_optimizer_steps`` is reached"""
        nonlocal acc
        tr.allreduce_grads(world)                           # the one exchange step of the path
        tr.lr = lr_at(tr.step_count, cfg)
        tr.step(world, max_grad_norm=cfg.max_grad_norm)
        mean_loss = D.max_over_ranks(acc, 1)                # local value; rank 0 logs
        losses.append(mean_loss)
        if log:
            log(dict(step=tr.step_count, loss=mean_loss, lr=tr.lr))
        acc = 0.0
        if output_dir and tr.step_count % save_steps == 0:
            CK.save_checkpoint(tr, output_dir, save_total_limit, rank, hf_config, tokenizer)
        return bool(max_optimizer_steps and tr.step_count >= max_optimizer_steps)

    for batch in batches:
        if cfg.pack_sequences:
            # the step's micro-batches, right padding stripped, as one stream of rows (data.plan_packed_step): one forward / backward
            pending.append(batch)
            micro += 1
            if micro % accum:
                continue
            from .data import plan_packed_step

            plan = plan_packed_step(pending, audio_cfg, pad_id)
            plan.segments = [(b, st, fr.to(engine.device, torch.float32)) for (b, st, fr) in plan.segments]
            loss = forward_backward_packed(plan, overlap_allreduce_world=world, last_micro_batch=cfg.max_grad_norm > 0)
            acc, pending = float(loss.item()), []
            if end_of_step():
                break
            continue
        ids = batch["input_ids"].to(engine.device)
        feats = batch.get("audio_encodings")
        if feats is not None:
            feats = [f.to(engine.device, torch.float32) for f in feats] if isinstance(feats, (list, tuple)) \
                else feats.to(engine.device, torch.float32)
        segs = plan_audio_splice(ids, feats, audio_cfg, False)
        labels = batch["labels"].to(engine.device)
        last = (micro + 1) % accum == 0                     # DDP no_sync boundary: exchange only on the last micro-step
        if fuse and accum > 1:
            pending.append((ids, segs, labels))
            if last:
                B = ids.shape[0]
                if len({tuple(p[0].shape) for p in pending}) == 1 and B * accum <= engine.max_batch:
                    all_segs = [(b + k * B, st, fr) for k, p in enumerate(pending) for (b, st, fr) in p[1]]
                    loss = forward_backward(torch.cat([p[0] for p in pending]), all_segs, torch.cat([p[2] for p in pending]), 1.0 / accum,
                                            overlap_allreduce_world=world, last_micro_batch=cfg.max_grad_norm > 0, loss_groups=accum)
                    acc = float(loss.item())
                else:                                       # ragged step (the collator pads each micro-batch to its own longest sequence)
                    for k, p in enumerate(pending):
                        acc += run_micro(*p, k == accum - 1)
                pending = []
        else:
            acc += run_micro(ids, segs, labels, last)
        micro += 1
        if micro % accum == 0 and end_of_step():
            break
    if output_dir:
        CK.save_checkpoint(tr, output_dir, save_total_limit, rank, hf_config, tokenizer)
    return losses


def check_supported_recipe(args) -> None:
    """Flags whose reference meaning the native loop does NOT implement must not be swallowed: a run that silently
    trains something else than asked is worse than no run.
      --lora_dropout > 0      : adapter dropout is not built (the reference's default is 0.05: pass 0.0 explicitly);
      --lora_bias != none     : biases do not train with the adapters;
      --lora_r                : a multiple of 8 up to 256 (the kernels pad the rank to a multiple of 64);
      --tune_mm_mlp_adapter False: the reference then leaves EVERY embedding row and lm_head trainable
                                (llamav2.py:395-419); the HIP trainer trains the two audio-token rows and freezes lm_head;
      --lr_scheduler_type     : only HF's cosine-with-warmup is implemented (train_llark.sh:35);
      --bf16 False            : the HIP training step is the bf16 flow;
      an MPT model name       : --freeze_backbone / --lora_enable / --gradient_checkpointing True (:func:`check_mpt_recipe`)."""
    if backbone_of(getattr(args, "model_name_or_path", "")) == "mpt":
        check_mpt_recipe(args)
    if getattr(args, "lora_enable", False):
        if float(getattr(args, "lora_dropout", 0.0)) != 0.0:
            raise NotImplementedError(f"--lora_dropout {args.lora_dropout}: adapter dropout is not implemented; pass --lora_dropout 0.0 "
                                      "(the reference's default is 0.05)")
        if str(getattr(args, "lora_bias", "none")) != "none":
            raise NotImplementedError(f"--lora_bias {args.lora_bias!r}: training biases with the adapters is not implemented (use 'none')")
        r = int(getattr(args, "lora_r", 64))
        if r <= 0 or r % 8 or r > 256:
            raise NotImplementedError(f"--lora_r {r}: the rank must be a multiple of 8 between 8 and 256")
    if not getattr(args, "tune_mm_mlp_adapter", True):
        raise NotImplementedError("--tune_mm_mlp_adapter False (all embedding rows + lm_head trainable) is not implemented: the HIP "
                                  "trainer updates the audio-token embedding rows only and keeps lm_head frozen")
    if getattr(args, "lr_scheduler_type", "cosine") != "cosine":
        raise NotImplementedError(f"--lr_scheduler_type {args.lr_scheduler_type!r}: only 'cosine' (with warm-up) is implemented")
    if not getattr(args, "bf16", True):
        raise NotImplementedError("--bf16 False: the HIP training step computes in the bf16 flow of the reference recipe")


def build_arg_parser():
    """The argument parser of :func:`main` (no model, tokenizer or GPU needed to build it)."""
    import argparse

    boolean = lambda v: str(v).lower() in ("1", "true", "yes")
    ap = argparse.ArgumentParser(description="LLark instruction tuning on the HIP training step")
    ap.add_argument("--model_name_or_path", required=True)
    ap.add_argument("--train_data_path", required=True)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--mm_hidden_size", type=int, default=4800)
    ap.add_argument("--mm_use_audio_start_end", type=boolean, default=True)
    ap.add_argument("--tune_mm_mlp_adapter", type=boolean, default=True)
    ap.add_argument("--per_device_train_batch_size", type=int, default=2)
    ap.add_argument("--gradient_accumulation_steps", type=int, default=4)
    ap.add_argument("--learning_rate", type=float, default=5e-5)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--warmup_ratio", type=float, default=0.03)
    ap.add_argument("--max_steps", type=int, default=100000)
    ap.add_argument("--model_max_length", type=int, default=2048)
    ap.add_argument("--save_steps", type=int, default=5000)
    ap.add_argument("--save_total_limit", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--grad_comm", default="bf16", choices=["fp32", "bf16"], help="transport dtype of the gradient all-reduce (reference: bf16)")
    ap.add_argument("--allow_pickle", type=boolean, default=False, help=".pyd shard members are pickles: enable only for trusted data")
    ap.add_argument("--fuse_accumulation", type=boolean, default=False,
                    help="not a reference flag: run the accumulation micro-batches of a step as one pass when they share a shape (same gradient; more HBM)")
    ap.add_argument("--pack_sequences", type=boolean, default=False,
                    help="not a reference flag: run the ragged micro-batches of a step as one packed stream (no pad rows, one pass over the weights; "
                         "same loss and gradient)")
    ap.add_argument("--gradient_checkpointing", type=boolean, default=False, help="train_llark.sh:25: recompute each decoder layer in the backward")
    ap.add_argument("--apply_task_sample_probs", type=boolean, default=False, help="m2t/arguments.py:68: weight shards by the task in their name")
    ap.add_argument("--task_sample_probs", default=None, help='JSON dict task -> probability (default: m2t/arguments.py:61-67)')
    ap.add_argument("--freeze_backbone", type=boolean, default=False,
                    help="m2t/train.py:79: train mm_projector and the audio-token embedding rows only")
    ap.add_argument("--lora_enable", type=boolean, default=False, help="m2t/train.py:82-99: LoRA adapters on a frozen base")
    ap.add_argument("--lora_r", type=int, default=64)
    ap.add_argument("--lora_alpha", type=float, default=16.0)
    ap.add_argument("--lora_dropout", type=float, default=0.0, help="only 0.0 is implemented (the reference's default is 0.05)")
    ap.add_argument("--lora_bias", default="none", help="only 'none' is implemented")
    ap.add_argument("--lr_scheduler_type", default="cosine")
    ap.add_argument("--bf16", type=boolean, default=True)
    ap.add_argument("--max_grad_norm", type=float, default=1.0, help="HF TrainingArguments.max_grad_norm (gradient clipping; 0 = off)")
    for ignored in ("--tf32", "--report_to", "--logging_steps", "--evaluation_strategy", "--save_strategy",
                    "--ddp_find_unused_parameters", "--dataloader_num_workers", "--num_train_epochs"):
        ap.add_argument(ignored, default=None, help="accepted for script compatibility (no effect on the arithmetic of the native loop)")
    return ap


def main(argv=None):
    """CLI with the flag names of ``m2t/train.py`` / ``scripts/training/train_llark.sh`` that the native loop implements:
    python -m llark_amd.m2t.train --model_name_or_path <hf dir> --train_data_path 'shards-{000..127}.tar' --output_dir out \
        --mm_hidden_size 4800 --mm_use_audio_start_end True --per_device_train_batch_size 2 --gradient_accumulation_steps 4 \
        --learning_rate 5e-5 --warmup_ratio 0.03 --max_steps 100000 --model_max_length 2048 --save_steps 5000 --save_total_limit 1
    (one process per GPU under ``python -m torch.distributed.run``).  A ``--model_name_or_path`` that contains "mpt" trains the MPT
    backbone (:func:`backbone_of`; scripts/training/train_mpt_model.sh)."""
    import torch as _torch
    from transformers import AutoTokenizer

    from .. import dist as D
    from .data import micro_batches
    args = build_arg_parser().parse_args(argv)
    check_supported_recipe(args)
    mpt = backbone_of(args.model_name_or_path) == "mpt"
    rank, world, local = D.env_rank_world()
    _torch.cuda.set_device(local)
    dev = _torch.device("cuda", local)
    if world > 1:
        D.init(backend="nccl", device=dev)
    tok = AutoTokenizer.from_pretrained(args.model_name_or_path, model_max_length=args.model_max_length, padding_side="right", use_fast=False)
    if tok.pad_token is None:
        tok.add_special_tokens(dict(pad_token="[PAD]"))                    # m2t/train.py:110-124
    if mpt:
        from .mpt import WrappedMPTForCausalLM

        model = WrappedMPTForCausalLM.from_pretrained(args.model_name_or_path, torch_dtype=_torch.bfloat16, mm_hidden_size=args.mm_hidden_size)
    else:
        from .llamav2 import WrappedLlamav2ForCausalLM

        model = WrappedLlamav2ForCausalLM.from_pretrained(args.model_name_or_path, torch_dtype=_torch.bfloat16)
    model.config.mm_hidden_size = args.mm_hidden_size
    model.get_model().initialize_adapter_modules(tune_mm_mlp_adapter=args.tune_mm_mlp_adapter)
    model.resize_token_embeddings(len(tok))
    model.initialize_audio_tokenizer(args.mm_use_audio_start_end, tok, device=dev, tune_mm_mlp_adapter=args.tune_mm_mlp_adapter)
    c = model.config
    if mpt:
        from .mpt_engine import HipMptEngine, MptDims

        a = c.attn_config
        dims = MptDims(d_model=c.d_model, n_heads=c.n_heads, n_layers=c.n_layers, expansion_ratio=c.expansion_ratio, vocab_size=len(tok),
                       max_seq_len=c.max_seq_len, alibi_bias_max=a["alibi_bias_max"], qk_ln=a["qk_ln"],
                       clip_qkv=a["clip_qkv"], logit_scale=model.logit_scale, mm_hidden_size=args.mm_hidden_size)
        # (--fuse_accumulation runs the per-micro-batch loop here: only the packed step needs a whole step's rows in the caches)
        eng = HipMptEngine(dims, dev, max_batch=args.per_device_train_batch_size * (args.gradient_accumulation_steps if args.pack_sequences else 1),
                           max_seq=args.model_max_length, precision="bf16")
    else:
        from .engine import HipLlamaEngine, LlamaDims

        dims = LlamaDims(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                         num_attention_heads=c.num_attention_heads, vocab_size=len(tok), rms_norm_eps=c.rms_norm_eps,
                         rope_theta=getattr(c, "rope_theta", 10000.0), mm_hidden_size=args.mm_hidden_size)
        fused_step = args.fuse_accumulation or args.pack_sequences           # the engine then holds a whole step's rows at once
        eng = HipLlamaEngine(dims, dev, max_batch=args.per_device_train_batch_size * (args.gradient_accumulation_steps if fused_step else 1),
                             max_seq=args.model_max_length, precision="bf16", frag_weights=False)
    eng.load_state_dict(model.state_dict())
    audio_cfg = model.get_model().audio_encoder_config
    hf_config = model.config                                              # written into every checkpoint-N (with the tokenizer)
    hf_config.mm_hidden_size = args.mm_hidden_size
    hf_config.tune_mm_mlp_adapter = args.tune_mm_mlp_adapter
    hf_config.mm_use_audio_start_end = args.mm_use_audio_start_end
    hf_config.vocab_size = len(tok)
    del model
    mm_cfg = dict(is_multimodal=True, sep_audio_conv_front=False, use_audio_start_end=args.mm_use_audio_start_end)
    cfg = TrainConfig(learning_rate=args.learning_rate, weight_decay=args.weight_decay, warmup_ratio=args.warmup_ratio,
                      max_steps=args.max_steps, gradient_accumulation_steps=args.gradient_accumulation_steps, grad_comm=args.grad_comm,
                      gradient_checkpointing=args.gradient_checkpointing, max_grad_norm=args.max_grad_norm,
                      fuse_accumulation=args.fuse_accumulation, pack_sequences=args.pack_sequences, freeze_backbone=args.freeze_backbone, lora_enable=args.lora_enable,
                      lora_r=args.lora_r, lora_alpha=args.lora_alpha, lora_dropout=args.lora_dropout, lora_bias=args.lora_bias,
                      seed=args.seed)
    task_probs = None
    if args.apply_task_sample_probs:
        import json as _json

        from .data import DEFAULT_TASK_SAMPLE_PROBS

        task_probs = _json.loads(args.task_sample_probs) if args.task_sample_probs else dict(DEFAULT_TASK_SAMPLE_PROBS)

    def batches(skip_micro_batches: int):
        return micro_batches(args.train_data_path, tok, mm_cfg, args.per_device_train_batch_size, args.model_max_length, rank, world,
                             seed=args.seed, allow_pickle=args.allow_pickle, skip_micro_batches=skip_micro_batches,
                             task_sample_probs=task_probs)

    log = (lambda rec: print(rec, flush=True)) if rank == 0 else None
    train(eng, batches, audio_cfg, cfg, world=world, max_optimizer_steps=args.max_steps, log=log, output_dir=args.output_dir,
          save_steps=args.save_steps, save_total_limit=args.save_total_limit, rank=rank, hf_config=hf_config, tokenizer=tok)
    D.shutdown(world)


if __name__ == "__main__":
    main()
