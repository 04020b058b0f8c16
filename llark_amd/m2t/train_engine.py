"""Training step of the LLM half on the HIP kernels: forward with saved activations, full backward, AdamW, and the
data-parallel gradient all-reduce (RCCL over xGMI via ``torch.distributed``; gloo in the CPU tests).

Replaces what the reference reaches through ``trainer.train()`` (m2t/train.py:255-260 -> HF ``Trainer.training_step``
-> ``WrappedLlamav2ForCausalLM.forward(labels=...)`` m2t/models/llamav2.py:259-337, ``loss.backward()``, DDP gradient
all-reduce, ``torch.optim.AdamW``; hyper-parameters scripts/training/train_llark.sh:20-49).

Semantics kept from the reference's default recipe (``--freeze_backbone False --tune_mm_mlp_adapter True --bf16 True``):
  * trainable: every Llama weight, ``mm_projector`` and -- through ``orig_embeds_params`` (m2t/models/llamav2.py:176-198)
    -- only the ``<audio_start>`` / ``<audio_end>`` rows of ``embed_tokens``; ``lm_head`` is frozen
    (m2t/models/llamav2.py:412-415);
  * bf16 parameters and matrix operands, fp32 accumulation; loss = mean shifted CE over labels != -100;
  * gradient accumulation over micro-batches (``--gradient_accumulation_steps``) then one AdamW step.
Differences (documented in DESIGN.md): AdamW moments are fp32 (torch keeps them in the parameter dtype); no
gradient checkpointing (288 GB of HBM hold the ~13 GB of saved activations of a 4 x 512 micro-batch).

Frozen-base recipes (``freeze_backbone=True``: m2t/train.py:79,146-148; ``lora=LoraConfig(...)``: m2t/train.py:82-99, peft LoraLayer
``y = W x + (alpha / r) B (A x)``): every base matrix, every norm gain and lm_head are frozen; the backward still carries dX through
every layer but computes no dW for them, and the parameter table, the flat gradient and the moments cover only what trains -- the
adapter factors (fp32 masters ``A^T [K][rp]`` / ``B [N][rp]``, bf16 operand copies rewritten after every step), mm_projector and
embed_tokens.  Where the operand twins exist the adapters ride in extra K columns of them (``[W | sB] [x ; A x]``: the fused RoPE / SwiGLU
epilogues are kept, only the tails are rewritten after a step); below FRAG_MIN_ROWS they run as separate low-rank products (csrc/lora.hip)
around the base products.

Gradients live in ONE flat fp32 buffer (views per tensor, kernel layouts: fused q|k|v rows, interleaved gate/up) so the
data-parallel exchange is a handful of large all-reduces.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops
from .engine import HipLlamaEngine
from .lora import LoraConfig, a_from_kernel, a_to_kernel, b_from_kernel, b_to_kernel, init_adapters, module_shape, parse_peft_key, peft_key

_BF = torch.bfloat16

# the fused weights of a decoder layer and the nn.Linear modules (LoRA targets) stored in each, with the first row and the stride
# between 32-row blocks of the module inside the fused matrix (gate / up rows are interleaved 32 by 32)
# Augmented K: the twin of a fused weight that carries its adapters in extra K columns, and which of the two twins it is.
# Slot 0, W fragment-major packed from [W | sb_diag]: y = [W | sB] [x ; A x] keeps the fused RoPE / SwiGLU forward epilogue.  Slot 1, W^T
# fragment-major packed from [W^T | a_cat]: dx = [dY | dT] [W ; A] keeps the fused SwiGLU backward / bf16 d(att) epilogue.
_AUG_SLOT = {"wqkv": ("qkv", 0), "wgu": ("gu", 0), "wo": ("o", 1), "wdown": ("down", 1)}
_LORA_GROUPS = (("qkv", "wqkv", ("q_proj", "k_proj", "v_proj")), ("o", "wo", ("o_proj",)),
                ("gu", "wgu", ("gate_proj", "up_proj")), ("down", "wdown", ("down_proj",)))
_GROUP_WEIGHT = {g: w for g, w, _ in _LORA_GROUPS}


class _LoraGroup:
    """The adapters of one fused weight [Ngrp][K]: fp32 masters per member (A^T [K][rp], B [N][rp]) and the bf16 operands of the four
    products, rewritten from the masters after every optimizer step (llark_lora_refresh; everything else in them stays zero):
      a_stack [nm rp][K]   : T = x . a_stack^T                     (llark_lora_down)
      sb_diag [Ngrp][nm rp]: y += T . sb_diag^T, member j's s B in its own rows and column block, zero elsewhere
      sb_t    [nm rp][Ngrp]: dT = dY . sb_t^T                      (llark_lora_down)
      a_cat   [K][nm rp]   : dx += dT . a_cat^T"""

    def __init__(self, layer: int, k: int, ngrp: int, rp: int, device):
        self.layer, self.k, self.ngrp, self.rp = layer, k, ngrp, rp
        self.members: list = []                  # (module, first row in the fused weight, 32-row block stride, N)
        self.device = device
        self.width = 0                           # nm rp: the K columns the adapters add to an augmented twin

    def allocate(self) -> None:
        w = self.width = len(self.members) * self.rp
        z = dict(dtype=_BF, device=self.device)
        self.a_stack = torch.zeros((w, self.k), **z)
        self.sb_diag = torch.zeros((self.ngrp, w), **z)
        self.sb_t = torch.zeros((w, self.ngrp), **z)
        self.a_cat = torch.zeros((self.k, w), **z)


class _Packing:
    """What a packed step (``forward_backward_packed``) changes in the body of ``forward_backward``: the rows are ONE stream (B = 1, S =
    s_total) cut into sequences by ``seqs`` = [(off, len)] (device table ``table``); RoPE of a row uses its position inside its sequence
    (``cos`` / ``sin``: the engine's tables gathered per row); the loss is normalised per group of rows (``groups`` = [(r0, r1)])."""

    def __init__(self, plan, eng):
        dev = eng.device
        self.seqs, self.groups, self.max_len, self.s_total = list(plan.seqs), list(plan.groups), plan.max_len, plan.s_total
        self.table = torch.tensor(self.seqs, dtype=torch.int32).to(dev)
        pos = plan.positions.to(dev)
        self.cos, self.sin = eng.cos.index_select(0, pos), eng.sin.index_select(0, pos)


class HipLlamaTrainer:
    def __init__(self, engine: HipLlamaEngine, lr: float = 5e-5, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, embed_grad_tokens: Sequence[int] = (), train_embed_all: bool = False,
                 grad_comm: torch.dtype = torch.float32, optimizer_state: bool = True, gradient_checkpointing: bool = False,
                 freeze_backbone: bool = False, lora: Optional[LoraConfig] = None, lora_seed: int = 0):
        if grad_comm not in (torch.float32, torch.bfloat16):
            raise ValueError("grad_comm must be torch.float32 or torch.bfloat16")
        self.grad_comm = grad_comm                   # transport dtype of the gradient all-reduce (the reference's DDP sends bf16)
        # train_llark.sh:25 `--gradient_checkpointing True` (HF: one checkpoint per decoder layer): the forward keeps only each
        # layer's input; the backward re-runs that layer's forward -- same kernels, same order, hence bit-identical gradients --
        # right before differentiating it.  Activation memory drops from ~0.18 MB to 16 KiB per token and layer at 7B widths.
        self.gradient_checkpointing = bool(gradient_checkpointing)
        if engine.split:
            raise ValueError("the training step runs in the reference's bf16 flow: build the engine with precision='bf16'")
        self.eng = engine
        engine.drop_frag_weights()                    # weights change in place from now on
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.embed_grad_tokens = set(int(t) for t in embed_grad_tokens)
        self.train_embed_all = train_embed_all
        self.step_count = 0
        d, dev = engine.dims, engine.device
        # m2t/train.py:79,146-148 `--freeze_backbone True` and :82-99 `--lora_enable True`: every base matrix, every norm gain and lm_head
        # are frozen -- the backward still carries dX through every layer but computes no dW for them, and the gradient / moment buffers
        # cover only what trains: the adapter factors (LoRA), mm_projector and embed_tokens (of which only the audio-token rows get a
        # gradient, as in the default recipe).
        self.lora = lora
        self.frozen = bool(freeze_backbone) or lora is not None
        self._matrices = {f"layers.{i}.{nm}": getattr(L, nm) for i, L in enumerate(engine.layers) for nm in ("wqkv", "wo", "wgu", "wdown")}
        # ---- parameter table: (name, tensor) in kernel layout; lm_head is frozen like the reference ----
        self.params: List[Tuple[str, torch.Tensor]] = []
        self._lora_groups: Dict[Tuple[int, str], _LoraGroup] = {}
        self.lora_flat: Optional[torch.Tensor] = None
        self.twins: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        self.lora_aug = False                          # (set below, before the twins are built: until then there is no tail to refresh)
        if self.frozen:
            if lora is not None:
                self._init_lora(lora, lora_seed)
            self.params.append(("embed", engine.embed))
        else:
            for i, L in enumerate(engine.layers):
                for nm in ("wqkv", "wo", "wgu", "wdown", "ln1", "ln2"):
                    self.params.append((f"layers.{i}.{nm}", getattr(L, nm)))
            self.params += [("norm", engine.norm), ("embed", engine.embed)]
        if engine.proj_w is not None:
            self.params += [("proj_w", engine.proj_w), ("proj_b", engine.proj_b)]
        self._pname = {p.data_ptr(): n for n, p in self._matrices.items()}
        self._pname.update({p.data_ptr(): n for n, p in self.params})
        total = sum(p.numel() for _, p in self.params)
        self.flat_grad = torch.zeros((total,), dtype=torch.float32, device=dev)
        # AdamW moments (2 x 27 GB at 7B): not allocated on the autograd-bridge path, where a torch optimizer owns the state
        self.flat_m = torch.zeros_like(self.flat_grad) if optimizer_state else None
        self.flat_v = torch.zeros_like(self.flat_grad) if optimizer_state else None
        self.grads: Dict[str, torch.Tensor] = {}
        self._slices: Dict[str, Tuple[int, int]] = {}
        off = 0
        for name, p in self.params:
            n = p.numel()
            self.grads[name] = self.flat_grad[off: off + n].view(p.shape)
            self._slices[name] = (off, n)
            off += n
        self.micro_batches = 0
        self._matrix_grads = {n for n, p in self.params if p.dim() == 2 and n != "embed"}
        self._fresh = set()                            # flat_grad starts zeroed: accumulate until the first zero_grad()
        # Operands DERIVED from the weights, valid until the next optimizer step (self._wver).  The first micro-batch of a step
        # needs none.  From the second micro-batch on, when there is something to amortise over, a fragment-major twin of W is
        # built once so that the forward products take the B-direct kernel like the inference engine (+8 .. 13 %); dX = dY . W
        # runs on W as stored (llark_gemm16_t) unless dx_direct_uses says otherwise.  Only when this object owns the optimizer:
        # on the autograd-bridge path the weights are rebuilt outside (sync_engine).
        self.derived_operands = bool(optimizer_state)
        self._wver = 0
        self._derived: Dict[int, list] = {}
        self._fwd_uses: Dict[int, list] = {}
        self._dx_uses: Dict[int, list] = {}
        # how many dX products per weight and optimizer step read W as it stands (llark_gemm16_t) before a K-contiguous W^T and
        # its fragment-major twin are built for the rest.  Default: all of them -- with the 128 x 256 tile llark_gemm16_t is within
        # 3 % of the B-direct kernel on these shapes, and the twins cost a transpose + a pack of all 13.5 GB of weights per step
        # (25 ms and 24 GB of HBM at 7B: 896 -> 868 ms for 4 micro-batches of 2 x 2048); they would pay from ~16 micro-batches.
        self.dx_direct_uses = int(os.environ.get("LLARK_TRAIN_DX_DIRECT_USES", str(1 << 30)))
        # Round 6: the optimizer itself keeps the operand twins current.  Every Llama weight matrix the twin kernel
        # takes carries TWO persistent fragment-major copies -- W (forward: the B-direct DMA loop from the FIRST micro-batch on) and W^T
        # (dX = dY . W on the same kernel instead of llark_gemm16_t) -- built once here and rewritten by llark_adamw_twins inside the
        # AdamW pass that already reads and writes every parameter (+ 4 B of stores on 22 B per parameter; no transpose16 / pack_frag in
        # the step).  +2 x 13.5 GB at 7B.  The q|k|v twin is stored in the fused-RoPE row order: the training forward takes
        # llark_gemm16_fragw_rope_qkv (RoPE, head split and both cache writes in the epilogue) wherever the shape qualifies.
        self._frozen_wT: Dict[int, torch.Tensor] = {}
        self._rope_order: Optional[torch.Tensor] = None          # gather index of the q|k|v twin's fused-RoPE row order
        self.use_twins = bool(optimizer_state) and os.environ.get("LLARK_TRAIN_TWINS", "1") != "0" and os.environ.get("LLARK_FRAG", "1") != "0"
        self.dw_fragw = os.environ.get("LLARK_TRAIN_DW_FRAGW", "1") != "0" and os.environ.get("LLARK_FRAG", "1") != "0"
        # the dW product on the 16x16x32 MFMA shape (csrc/gemm_bda16.hip): more flops per joule under the power limit
        self.dw_mfma16 = self.dw_fragw and os.environ.get("LLARK_TRAIN_DW_MFMA16", "0") != "0"
        self.attn_glue_fused = os.environ.get("LLARK_TRAIN_ATTN_GLUE_FUSED", "1") != "0"
        self.swiglu_fused = self.use_twins and os.environ.get("LLARK_TRAIN_SWIGLU_FUSED", "1") != "0"
        self.rope_fused = self.use_twins and d.head_dim == 128 and d.num_attention_heads % 2 == 0 and os.environ.get("LLARK_TRAIN_ROPE_FUSED", "1") != "0"
        self.lora_aug = self.use_twins and os.environ.get("LLARK_TRAIN_LORA_AUG", "1") != "0"   # 0: separate products everywhere (measurement)
        if not self.lora_aug and any(g == "qkv" for _, g in self._lora_groups):
            # separate products: the adapters' share of q | k | v is added BEFORE the rotation, the product keeps its fp32 output
            self.rope_fused = False
        self._ln_sink = torch.zeros((d.hidden_size,), dtype=torch.float32, device=dev) if self.frozen else None   # frozen gains: dgain goes nowhere
        if self.use_twins:
            self._build_twins()
        # gradient-norm bookkeeping (HF Trainer max_grad_norm): sum of squares collected by the dW epilogues of a step's last
        # micro-batch, the flat-gradient spans it already covers, and the total of the last clipped step
        self._norm_collect = False
        self._norm_acc: Optional[torch.Tensor] = None
        self._norm_spans: List[Tuple[int, int]] = []
        self._last_sumsq: Optional[torch.Tensor] = None
        self._exchange_events: list = []
        self.time_phases = False                  # True: forward_backward leaves (start, forward done, backward done) HIP events in phase_events
        self.phase_events: Optional[list] = None

    # ------------------------------------------------------------------------------------------
    def zero_grad(self) -> None:
        """Weight-matrix gradients are WRITTEN by the first micro-batch's dW product (no 27 GB memset, no residual read
        in that epilogue); only the small accumulate-only slices (norm gains, embedding rows, projector bias) are zeroed."""
        for name, _ in self.params:
            if name not in self._matrix_grads:
                self.grads[name].zero_()
        self._fresh = set(self._matrix_grads)
        self.micro_batches = 0

    def _build_twins(self) -> None:
        """Initial construction of the operand twins (afterwards llark_adamw_twins rewrites them with every optimizer step)."""
        eng, d = self.eng, self.eng.dims
        H = d.hidden_size
        for i, L in enumerate(eng.layers):
            for nm in ("wqkv", "wo", "wgu", "wdown"):
                w = getattr(L, nm)
                n, k = w.shape
                if not ops.adamw_twins_takes(n, k) or not w.is_contiguous():
                    continue
                rope_rows = 2 * H if (nm == "wqkv" and self.rope_fused) else 0
                # (frozen base: built here once and never rewritten -- no optimizer pass touches these matrices)
                self.twins[f"layers.{i}.{nm}"] = self._pack_twins(w, rope_rows, aug=self._aug_of(f"layers.{i}.{nm}")) + (rope_rows,)
        # lm_head is frozen (m2t/models/llamav2.py:412-415): its twins go stale only when the weights are loaded from outside
        lm = eng.lm_head
        if lm is not None and lm.shape[1] % 64 == 0:
            ops.attach_frag(lm, lm.shape[0])
            wT = ops.transposed16(lm)                             # [H][V padded to 64]
            ops.attach_frag(wT, wT.shape[0])
            self._frozen_wT[lm.data_ptr()] = wT

    def _aug_of(self, name: str):
        """(adapter group, twin slot) of a matrix whose twin carries its adapters in extra K columns (_AUG_SLOT), else None."""
        _, i, nm = name.split(".")
        gname, slot = _AUG_SLOT[nm]
        g = self._lora_groups.get((int(i), gname)) if self.lora_aug else None
        return None if g is None else (g, slot)

    def _pack_twins(self, w: torch.Tensor, rope_rows: int, wfrag: Optional[torch.Tensor] = None,
                    wtfrag: Optional[torch.Tensor] = None, aug=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """W fragment-major (in the fused-RoPE row order when ``rope_rows``) and W^T fragment-major; into ``wfrag`` / ``wtfrag`` when given.
        ``aug`` = (group, slot): that twin is packed from [W | sb_diag] (slot 0) or [W^T | a_cat] (slot 1) of the group's current operands."""
        n, k = w.shape
        g, slot = aug if aug is not None else (None, -1)
        src = torch.cat((w, g.sb_diag), dim=1) if slot == 0 else w
        if rope_rows:
            if self._rope_order is None:
                self._rope_order = ops.rope_qkv_row_order(self.eng.dims.num_attention_heads, self.eng.dims.head_dim).to(w.device)
            wfrag = ops.pack_weight16_frag(src.index_select(0, self._rope_order), n, out=wfrag)
        else:
            wfrag = ops.pack_weight16_frag(src, n, out=wfrag)
            if slot != 0:
                w._llark_frag = (wfrag, n, k)                     # ops.gemm16 takes the B-direct kernel for >= FRAG_MIN_ROWS rows
        del src
        wT = ops.transposed16(w)                                  # [k][n] (n % 64 == 0: no padding)
        if slot == 1:
            wT = torch.cat((wT, g.a_cat), dim=1)
        wtfrag = ops.pack_weight16_frag(wT, k, out=wtfrag)
        del wT
        return wfrag, wtfrag

    def refresh_derived(self) -> None:
        """The weights were overwritten in place from outside the optimizer (checkpoint.load_checkpoint): every operand twin is
        re-packed into its own buffers, the lm_head operands are rebuilt from ``eng.lm_head``, and the per-step caches are
        invalidated as after an optimizer step.  Otherwise the next step would compute with the weights the twins were built from."""
        for name, (wfrag, wtfrag, rope_rows) in self.twins.items():
            self._pack_twins(self._matrices[name], rope_rows, wfrag, wtfrag, aug=self._aug_of(name))
        lm = self.eng.lm_head
        wT = self._frozen_wT.get(lm.data_ptr()) if lm is not None else None
        if wT is not None:
            ops.refresh_frag(lm)
            ops.transpose16(lm, lm.stride(0), lm.shape[0], lm.shape[1], wT, wT.shape[1])
            ops.refresh_frag(wT)
        self._refresh_lora()
        self._weights_changed(base=True)

    # ---- LoRA adapters ------------------------------------------------------------------------------
    def _init_lora(self, cfg: LoraConfig, seed: int) -> None:
        """Allocates the fp32 masters of every adapter pair in ONE flat buffer (the head of the parameter table: a single AdamW launch
        covers them, layer by layer contiguous for the overlapped all-reduce) and the bf16 operands of every group."""
        d, dev = self.eng.dims, self.eng.device
        H, I, rp = d.hidden_size, d.intermediate_size, cfg.rp
        specs = []
        for i, L in enumerate(self.eng.layers):
            for gname, wname, mods in _LORA_GROUPS:
                ngrp, k = getattr(L, wname).shape
                grp = None
                for j, mod in enumerate(mods):
                    if mod not in cfg.target_modules:
                        continue
                    if grp is None:
                        grp = _LoraGroup(i, k, ngrp, rp, dev)
                    n, _ = module_shape(mod, H, I)
                    row0, blk = (32 * j, 64) if gname == "gu" else (j * n, 32)
                    grp.members.append((mod, row0, blk, n))
                    specs += [(f"layers.{i}.{mod}.lora_At", (k, rp)), (f"layers.{i}.{mod}.lora_B", (n, rp))]
                if grp is not None:
                    if k % 32 or ngrp % 32:
                        raise ValueError(f"lora: layer widths {ngrp} x {k} must be multiples of 32")
                    grp.allocate()
                    self._lora_groups[(i, gname)] = grp
        self.lora_flat = torch.zeros((sum(a * b for _, (a, b) in specs),), dtype=torch.float32, device=dev)
        off = 0
        for name, (a, b) in specs:
            self.params.append((name, self.lora_flat[off: off + a * b].view(a, b)))
            off += a * b
        self.set_adapters(init_adapters(cfg, H, I, d.num_hidden_layers, seed))

    def set_adapters(self, adapters: Dict[str, torch.Tensor]) -> None:
        """Loads adapter factors given under peft names (``...q_proj.lora_A.weight`` [r][K], ``lora_B.weight`` [N][r]) into the fp32
        masters (A transposed, rank zero-padded) and rewrites the bf16 operands."""
        cfg, params = self.lora, dict(self.params)
        want = {peft_key(g.layer, m[0], w) for g in self._lora_groups.values() for m in g.members for w in "AB"}
        if set(adapters) != want:
            odd = sorted(set(adapters) ^ want)
            raise KeyError(f"adapter keys do not match this trainer's targets: {odd[:3]}{'...' if len(odd) > 3 else ''}")
        for key, t in adapters.items():
            layer, mod, which = parse_peft_key(key)
            dst = params[f"layers.{layer}.{mod}.lora_" + ("At" if which == "A" else "B")]
            src = (a_to_kernel if which == "A" else b_to_kernel)(t.to(dst.device), cfg.rp)
            if src.shape != dst.shape:
                raise ValueError(f"{key}: shape {tuple(t.shape)} does not fit r={cfg.r}")
            dst.copy_(src)
        self._refresh_lora()

    def get_adapters(self) -> Dict[str, torch.Tensor]:
        """The adapter factors under peft names, unpadded rank (fp32 copies)."""
        return self._adapters_from(dict(self.params))

    def _adapters_from(self, table: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        out = {}
        for g in self._lora_groups.values():
            for mod, _, _, _ in g.members:
                out[peft_key(g.layer, mod, "A")] = a_from_kernel(table[f"layers.{g.layer}.{mod}.lora_At"], self.lora.r)
                out[peft_key(g.layer, mod, "B")] = b_from_kernel(table[f"layers.{g.layer}.{mod}.lora_B"], self.lora.r)
        return out

    def _refresh_lora(self) -> None:
        """bf16 operands <- fp32 masters (llark_lora_refresh writes the adapters' own blocks only)."""
        if not self._lora_groups:
            return
        params, rp, s = dict(self.params), self.lora.rp, self.lora.scale
        for g in self._lora_groups.values():
            for j, (mod, row0, blk, n) in enumerate(g.members):
                c0, c1 = j * rp, (j + 1) * rp
                ops.lora_refresh(params[f"layers.{g.layer}.{mod}.lora_At"], 1.0, g.a_cat[:, c0:c1], g.a_stack[c0:c1], 32)
                ops.lora_refresh(params[f"layers.{g.layer}.{mod}.lora_B"], s, g.sb_diag[row0:, c0:c1], g.sb_t[c0:c1, row0:], blk)
        # the adapters' K columns of the augmented twins.  Fragment-major = 1-KiB chunks [32-row tile][16-wide k step], so those columns are
        # one contiguous run of chunks per row tile: the small operand is packed on its own and copied over that run; the frozen chunks
        # are neither read nor written.
        for (i, gname), g in self._lora_groups.items():
            name = f"layers.{i}.{_GROUP_WEIGHT[gname]}"
            tw, aug = self.twins.get(name), self._aug_of(name)
            if tw is None or aug is None:
                continue
            slot = aug[1]
            small, nrows, kbase = (g.sb_diag, g.ngrp, g.k) if slot == 0 else (g.a_cat, g.k, g.ngrp)
            if slot == 0 and tw[2]:
                small = small.index_select(0, self._rope_order)
            tail = ops.pack_weight16_frag(small, nrows)
            tw[slot].view(nrows // 32, (kbase + g.width) // 16, 512)[:, kbase // 16:].copy_(tail.view(nrows // 32, g.width // 16, 512))

    def _norm_aug(self, h: torch.Tensor, gain: torch.Tensor, g: Optional[_LoraGroup], st: dict, key: str):
        """RMSNorm(h) as the bf16 A operand of the next product.  With an adapter group ``g`` the buffer is [rows][K + nm rp] and its tail
        holds T = x A^T (llark_lora_down), saved under ``st[key]``.  Returns (x [rows][K], the whole buffer)."""
        rows, H = h.shape
        xw = torch.empty((rows, H + (g.width if g is not None else 0)), dtype=_BF, device=h.device)
        ops.rmsnorm_bf16(h, gain, self.eng.dims.rms_norm_eps, xw)
        if g is None:
            return xw, xw
        x = xw[:, :H]
        st[key] = xw[:, H:]
        ops.lora_down(x, g.a_stack, st[key])
        return x, xw

    def _lora_fwd(self, g: _LoraGroup, x16: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """y [rows][Ngrp] fp32 (the base product, bias-free) += (x A^T) (s B)^T for every member; returns T = x A^T (bf16, saved)."""
        t = torch.empty((x16.shape[0], g.a_stack.shape[0]), dtype=_BF, device=x16.device)
        ops.lora_down(x16, g.a_stack, t)
        ops.gemm16(t, None, g.sb_diag, None, g.ngrp, ops.EPI_RESID, c=y, resid=y)
        return t

    def _lora_bwd(self, g: _LoraGroup, dy16: torch.Tensor, x16: torch.Tensor, t: torch.Tensor, dx: Optional[torch.Tensor],
                  dt: Optional[torch.Tensor] = None) -> None:
        """The adapters' share of a group's backward: dT = dY (s B) (``dt``: the caller has it already); dB (+)= s dY^T T and
        dA^T (+)= x^T dT per member (llark_lora_dw); dx [rows][K] fp32 (holding dY . W of the frozen base) += dT A (``dx`` None: the
        caller's augmented product covers it)."""
        rp, r, s = g.rp, self.lora.r, self.lora.scale
        if dt is None:
            dt = torch.empty(t.shape, dtype=_BF, device=t.device)
            ops.lora_down(dy16, g.sb_t, dt, k=g.ngrp)
        sumsq = self._norm_acc if self._norm_collect else None
        for j, (mod, row0, blk, n) in enumerate(g.members):
            c0, c1 = j * rp, (j + 1) * rp
            for name, p, q, scale, pb in ((f"layers.{g.layer}.{mod}.lora_B", dy16[:, row0:], t[:, c0:c1], s, blk),
                                          (f"layers.{g.layer}.{mod}.lora_At", x16, dt[:, c0:c1], 1.0, 32)):
                fresh = name in self._fresh
                self._fresh.discard(name)
                ops.lora_dw(p, q, self.grads[name], r, scale, accumulate=not fresh, sumsq=sumsq, p_blk=pb)
                if sumsq is not None:
                    off, cnt = self._slices[name]
                    self._norm_spans.append((off, off + cnt))
        if dx is not None:
            ops.gemm16(dt, None, g.a_cat, None, g.k, ops.EPI_RESID, c=dx, resid=dx)

    def _twin_of(self, w: torch.Tensor):
        name = self._pname.get(w.data_ptr())
        return self.twins.get(name) if name is not None else None

    def _dw(self, dy16: torch.Tensor, x16: torch.Tensor, grad: torch.Tensor, name: str) -> None:
        """grad[N][K] (+)= dY^T . X   (dy16 [rows][N], x16 [rows][K] bf16); plain write on the first micro-batch.
        Both operands are contraction-major as they stand (the token index is their row): ``llark_gemm16_t`` reads them through
        the transposing LDS load, no dY^T / X^T copies; token counts that are not a multiple of 64 take the transposing path.
        On the last micro-batch of a step (``_norm_collect``) the product's epilogue also adds the sum of squares of the gradient
        it completes to ``_norm_acc`` (gradient-norm clipping without re-reading the gradients)."""
        sumsq = self._norm_acc if self._norm_collect else None
        n, k = dy16.shape[1], x16.shape[1]
        fresh = name in self._fresh
        self._fresh.discard(name)
        toks = dy16.shape[0]
        if (self.dw_fragw and toks >= ops.FRAG_MIN_ROWS and x16.shape[0] == toks and k % 8 == 0 and x16.stride(0) % 8 == 0
                and ops.gemm16_ta_fragw_takes(n, toks, dy16.stride(0))):
            # round 6: dY as it stands through the DMA loop's transposing LDS read, X^T fragment-major (one transposing pack of X: 2 x its
            # bytes) -- the B operand streams L2 -> VGPR and never waits on a barrier (csrc/gemm_bda.hip: gemm_bda_ta_kernel)
            c16 = self.dw_mfma16 and ops.gemm16_ta_fragw16_takes(n, k, toks, dy16.stride(0), grad)
            xt = ops.pack_frag_t16(x16, k, chunk16=c16)
            ops.gemm16_ta_fragw(dy16, xt, n, k, toks, grad, accumulate=not fresh, sumsq=sumsq, chunk16=c16)
            if sumsq is not None:
                off, cnt = self._slices[name]
                self._norm_spans.append((off, off + cnt))
            return
        if dy16.shape[0] % 64 == 0 and n % 8 == 0 and k % 8 == 0 and dy16.stride(0) % 8 == 0 and x16.stride(0) % 8 == 0:
            ops.gemm16_t(dy16, x16, n, k, dy16.shape[0], True, True, grad, accumulate=not fresh, sumsq=sumsq)
            if sumsq is not None:                          # this gradient's share of the squared norm is in the accumulator already
                off, cnt = self._slices[name]
                self._norm_spans.append((off, off + cnt))
            return
        dyT = ops.transposed16(dy16)
        xT = ops.transposed16(x16)
        if fresh:
            ops.gemm16(dyT, None, xT, None, k, ops.EPI_F32, c=grad, m=n)
        else:
            ops.gemm16(dyT, None, xT, None, k, ops.EPI_RESID, c=grad, resid=grad, m=n)

    def _w_transposed(self, w: torch.Tensor) -> torch.Tensor:
        """The K-contiguous W^T of a dX product that does not go through llark_gemm16_t (shapes it does not take, or -- with
        ``derived_operands`` -- the second and later micro-batches of an optimizer step, which share one W^T with a fragment-major
        twin for the B-direct kernel)."""
        if not self.derived_operands:
            return ops.transposed16(w)
        ent = self._derived.get(w.data_ptr())
        if ent is None or ent[0] != self._wver:
            ent = [self._wver, ops.transposed16(w)]
            self._derived[w.data_ptr()] = ent
            if ent[1].shape[1] % 64 == 0:
                ops.attach_frag(ent[1], ent[1].shape[0])
        return ent[1]

    def _fwd_weight(self, w: torch.Tensor) -> torch.Tensor:
        """A weight about to be multiplied in a forward product: from its second use since the last optimizer step it carries a
        fragment-major twin (ops.gemm16 then takes the B-direct kernel)."""
        if self.twins and self._twin_of(w) is not None:
            return w
        if self.derived_operands:
            ent = self._fwd_uses.get(w.data_ptr())
            if ent is None or ent[0] != self._wver:
                ent = [self._wver, 0]
                self._fwd_uses[w.data_ptr()] = ent
            ent[1] += 1
            if ent[1] == 2 and w.shape[1] % 64 == 0:
                ops.attach_frag(w, w.shape[0])
        return w

    def _weights_changed(self, base: bool = False) -> None:
        """After an optimizer step: every derived operand is stale.  With a frozen base the operands derived from the base matrices
        outlive the step (``base``: they were overwritten from outside, refresh_derived)."""
        if self.frozen and not base:
            # Invariant: ``_wver`` versions operands derived from the BASE matrices and lm_head only (_fwd_weight, _w_transposed, _dx) --
            # none of the trainable tensors of a frozen run (embed, proj_w, proj_b, the adapter masters) goes through them, so the version
            # stands still here.  proj_w's only derived operand is the fragment-major twin ops.gemm16 attaches; it is dropped below.
            # Whoever routes a trainable tensor through those caches has to bump ``_wver`` here as well.
            if self.derived_operands and self.eng.proj_w is not None:
                ops.detach_frag(self.eng.proj_w)
            return
        self._wver += 1
        if self.derived_operands:
            for n, p in list(self.params) + (list(self._matrices.items()) if self.frozen else []):
                if p.dim() == 2 and n not in self.twins:
                    ops.detach_frag(p)

    def _dx(self, dy16: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> None:
        """out[rows][K] = dY . W   (w [N][K] bf16 kernel layout: its row IS the contraction index).
        ``llark_gemm16_t`` on W as it stands (no W^T) for the first ``dx_direct_uses`` products of a weight since the last optimizer
        step -- by default all of them; past that the K-contiguous transpose + fragment-major twin are built once and the B-direct
        kernel (~3 % faster per product) amortises them over the remaining micro-batches."""
        n, k = w.shape
        rows = dy16.shape[0]
        if not dy16.is_contiguous():                   # (the head of a [dY | dT] buffer whose augmented product was not taken)
            dy16 = dy16.contiguous()
        if rows >= ops.FRAG_MIN_ROWS and dy16.stride(0) % 8 == 0:
            tw = self._twin_of(w)
            if tw is not None and dy16.shape[1] >= n and tw[1].numel() == n * k:   # W^T fragment-major, kept current by llark_adamw_twins
                # (an augmented W^T twin also contracts over the adapters' dT columns: its callers pass [dY | dT] themselves)
                ops.gemm16_fragw(dy16, None, tw[1], None, k, n, ops.EPI_F32, c=out)
                return
            wT = self._frozen_wT.get(w.data_ptr())
            if wT is not None and dy16.shape[1] >= wT.shape[1]:
                ops.gemm16(dy16, None, wT, None, k, ops.EPI_F32, c=out)
                return
        if self.derived_operands:
            ent = self._dx_uses.get(w.data_ptr())
            if ent is None or ent[0] != self._wver:
                ent = [self._wver, 0]
                self._dx_uses[w.data_ptr()] = ent
            ent[1] += 1
            first = ent[1] <= self.dx_direct_uses
        else:
            first = True
        if first and n % 64 == 0 and k % 8 == 0 and dy16.shape[1] >= n and dy16.stride(0) % 8 == 0:
            ops.gemm16_t(dy16, w, dy16.shape[0], k, n, False, True, out)
            return
        wT = self._w_transposed(w)                    # [K][Np]
        if dy16.shape[1] < wT.shape[1]:               # pad dY columns up to the 64-multiple K of this product
            pad = torch.zeros((dy16.shape[0], wT.shape[1]), dtype=_BF, device=dy16.device)
            pad[:, : dy16.shape[1]] = dy16
            dy16 = pad
        ops.gemm16(dy16, None, wT, None, w.shape[1], ops.EPI_F32, c=out)

    # ------------------------------------------------------------------------------------------
    def forward_backward_packed(self, seqs, segs, labels, groups, loss_scale: Optional[float] = None, overlap_allreduce_world: int = 1,
                                last_micro_batch: bool = False, pad_id: int = 0, plan=None) -> torch.Tensor:
        """A whole optimizer step of ragged sequences as ONE packed stream: no padded sequence, one pass over the weights.
        ``seqs`` / ``labels``: lists of 1-D id / label tensors of any lengths; ``segs``: (sequence index, start, frames) as in
        :meth:`forward_backward`; ``groups``: the number of sequences in each micro-batch of the step.  The loss keeps the reference's
        meaning -- each micro-batch's mean cross-entropy over ITS shifted targets, averaged over the micro-batches (``loss_scale``
        defaults to 1 / len(groups)) -- so the gradient is the sum the separate right-padded micro-batches would accumulate.
        Every sequence is padded to a multiple of 8 rows with ``pad_id`` / label -100 (data.pack_sequences; ``plan``: a PackedStep
        built already, e.g. by data.plan_packed_step); attention runs on the variable-length kernels (llark_attn_*_varlen), RoPE uses
        the position inside the sequence, and each layer's saved K / V^T live in that layer's own cache memory viewed as one sequence
        of s_total positions."""
        from .data import pack_sequences

        if plan is None:
            plan = pack_sequences(seqs, labels, groups, segs, pad_id)
        eng = self.eng
        if plan.s_total > eng.max_batch * eng.smax:
            raise ValueError(f"forward_backward_packed: s_total = {plan.s_total} packed rows do not fit the engine's caches "
                             f"(max_batch * smax = {eng.max_batch} * {eng.smax} positions)")
        if plan.max_len > eng.cos.shape[0]:
            raise ValueError(f"forward_backward_packed: a sequence of {plan.max_len} rows is beyond the RoPE table ({eng.cos.shape[0]} positions)")
        if eng.dims.head_dim != 128:
            raise ValueError("forward_backward_packed: the variable-length attention kernels need head_dim 128")
        return self.forward_backward(plan.ids.view(1, -1).to(eng.device), plan.segments, plan.labels.view(1, -1),
                                     1.0 / len(plan.groups) if loss_scale is None else loss_scale, overlap_allreduce_world, last_micro_batch,
                                     _packing=_Packing(plan, eng))

    def forward_backward(self, input_ids: torch.Tensor, audio_segments, labels: torch.Tensor, loss_scale: float = 1.0,
                         overlap_allreduce_world: int = 1, last_micro_batch: bool = False, loss_groups: int = 1,
                         _packing: Optional[_Packing] = None) -> torch.Tensor:
        """One micro-batch: returns the (unscaled) loss as a device scalar and ACCUMULATES gradients.
        ``loss_scale`` = 1 / gradient_accumulation_steps like HF Trainer.
        ``loss_groups`` > 1: the batch holds that many of the recipe's micro-batches (consecutive, equal-sized groups of sequences) run
        as ONE pass -- the accumulation of train_llark.sh:26-27 (per_device_train_batch_size 2 x gradient_accumulation_steps 4) fused:
        the loss is normalised per group (each group's mean over ITS label tokens, times ``loss_scale``), so the gradient is the sum the
        separate micro-batches would accumulate; every dW product then writes its gradient once instead of read-modify-writing 27 GB of
        fp32 per micro-batch.  Returns the mean of the group losses.
        ``last_micro_batch``: this call completes the gradients of an optimizer step: every dW product then also adds the sum of
        squares of the gradient it writes to a device scalar (epilogue of ``llark_gemm16_t_sumsq``) -- ``step(max_grad_norm=...)``
        only reduces what is left (norm gains, embedding rows) instead of re-reading all 27 GB of gradients.  (Single rank only: with
        an all-reduce pending the norm is taken after it, in one pass.)
        ``overlap_allreduce_world`` > 1 (pass it on the LAST micro-batch of an optimizer step, the reference's DDP
        ``no_sync`` boundary): as soon as the backward of decoder layer i is complete its ~0.8 GB gradient slice is
        all-reduced asynchronously (RCCL stream) while layers i-1 ... 0 are still being differentiated; call
        :meth:`allreduce_grads` afterwards -- it only exchanges what is left and waits."""
        eng, d = self.eng, self.eng.dims
        dev = eng.device
        B, S = input_ids.shape
        # last micro-batch on one rank: every dW product also leaves the sum of squares of the gradient it completes (epilogue of
        # llark_gemm16_t_sumsq), so step(max_grad_norm=...) only has to reduce the small rest instead of re-reading 27 GB
        self._norm_collect = bool(last_micro_batch and self.flat_m is not None and overlap_allreduce_world <= 1)
        if self._norm_collect:
            if self._norm_acc is None:
                self._norm_acc = torch.zeros((1,), dtype=torch.float64, device=self.flat_grad.device)
            self._norm_acc.zero_()
        # a collecting call starts from scratch; any OTHER call adds to gradients whose squares an earlier collecting call may
        # have summed: those partial sums are stale either way
        self._norm_spans = []
        ev = None
        if getattr(self, "time_phases", False) and self.flat_grad.is_cuda:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]        # start | forward done | backward done
            ev[0].record()
        rows = B * S
        H, I, nh, hd, V = d.hidden_size, d.intermediate_size, d.num_attention_heads, d.head_dim, d.vocab_size
        f32 = dict(dtype=torch.float32, device=dev)
        bf = dict(dtype=_BF, device=dev)
        pk = _packing                                                   # a packed step (forward_backward_packed): B = 1, S = s_total
        eng.reset(B if pk is None else eng.max_batch)
        if pk is None:
            smax = eng.smax
            caches = lambda i: (eng.k_cache[i, :B], eng.vt_cache[i, :B])            # [B][nh][smax][hd], [B][nh][hd][smax]
            cos, sin = eng.cos, eng.sin
        else:
            # the caches are scratch during training: a layer's saved K / V^T are ONE sequence of S positions at the head of its own memory
            smax = S
            caches = lambda i: (eng.k_cache[i].view(-1)[: nh * S * hd].view(1, nh, S, hd), eng.vt_cache[i].view(-1)[: nh * S * hd].view(1, nh, hd, S))
            cos, sin = pk.cos, pk.sin                                   # row r rotates by its position inside its sequence
        ids_flat = input_ids.reshape(-1).contiguous()
        h = torch.empty((rows, H), **f32)
        ops.embed_gather(ids_flat, eng.embed, h)
        seg_rows, seg_a16 = [], []
        for (b, start, frames) in audio_segments:
            F = frames.shape[0]
            a16, _ = ops.split16(frames.contiguous(), _BF, want_lo=False, kmult=64)
            r0 = (b * S if pk is None else pk.seqs[b][0]) + start + 1
            ops.gemm16(a16, None, eng.proj_w, eng.proj_b, H, ops.EPI_F32, c=h[r0: r0 + F])
            seg_rows.append(torch.arange(r0, r0 + F, device=dev))
            seg_a16.append(a16[:, : d.mm_hidden_size])
        fused_rows = rows >= ops.FRAG_MIN_ROWS                          # the fragment-major (B-direct) kernels take the products
        # round 6: every RMSNorm backward also leaves the bf16 copy of its dx (the next products' A operand): no split16 pass over dh
        fuse16 = H % 64 == 0 and os.environ.get("LLARK_TRAIN_NORM_BWD_OUT16", "1") != "0"
        # ---------------- forward, saving what the backward needs ----------------
        def layer_forward(i, L, h):
            """One decoder layer on the residual stream ``h`` (updated in place); returns everything its backward reads."""
            st = {"h_in": h}                                       # the stream is never updated in place: each residual product writes a new buffer
            lg = self._lora_groups
            tw = self.twins.get(f"layers.{i}.wqkv")
            fused_qkv = tw is not None and tw[2] and S >= 32 and fused_rows
            # augmented K: x1 = [RMSNorm(h) | T] with T = x A^T in the tail columns, against the [W | sB] twin
            x1, x1w = self._norm_aug(h, L.ln1, lg.get((i, "qkv")) if fused_qkv and self.lora_aug else None, st, "t_qkv")
            q = torch.empty((B, nh, S, hd), **bf)
            kc, vc = caches(i)
            v_rm = None
            if fused_qkv:                                                # RoPE / head split / K and V^T writes in the product's epilogue
                if self.attn_glue_fused:                                 # ... and V row-major for the backward (no transpose16 of the V^T cache)
                    v_rm = torch.empty((B * nh, S, hd), **bf)
                    ops.gemm16_fragw_rope_qkv_train(x1w, tw[0], x1w.shape[1], B, S, nh, 0, cos, sin, q, kc, vc, v_rm)
                else:
                    ops.gemm16_fragw_rope_qkv(x1w, None, tw[0], x1w.shape[1], B, S, nh, 0, cos, sin, q, kc, vc)
            else:
                qkv = torch.empty((rows, 3 * H), **f32)
                ops.gemm16(x1, None, self._fwd_weight(L.wqkv), None, 3 * H, ops.EPI_F32, c=qkv)
                if (i, "qkv") in lg:
                    st["t_qkv"] = self._lora_fwd(lg[(i, "qkv")], x1, qkv)
                ops.rope_split_heads(qkv, B, S, nh, hd, 0, cos, sin, q, kc, vc)
                del qkv
            att = torch.empty((rows, H), **bf)
            lse = torch.empty((B * nh, S), **f32)                         # per-query log-sum-exp: the backward recomputes P from it
            if pk is None:
                ops.attn_prefill_lse(q, kc, vc, B, S, nh, hd, att, lse)
            else:
                ops.attn_prefill_lse_varlen(q, kc, vc, pk.table, pk.seqs, pk.max_len, S, nh, hd, att, lse)
            h_mid = torch.empty_like(h)
            ops.gemm16(att, None, self._fwd_weight(L.wo), None, H, ops.EPI_RESID, c=h_mid, resid=h)
            if (i, "o") in lg:
                st["t_o"] = self._lora_fwd(lg[(i, "o")], att, h_mid)
            h = h_mid
            st.update(x1=x1, q=q, att=att, lse=lse, h_mid=h_mid, v_rm=v_rm)
            act = torch.empty((rows, I), **bf)
            tw = self.twins.get(f"layers.{i}.wgu")
            gu = None
            # (separate products: the adapters' shares enter before SwiGLU / its backward, which then need the fp32 gate | up)
            fused_gu = (tw is not None and fused_rows and self.swiglu_fused and self.twins.get(f"layers.{i}.wdown") is not None
                        and (self.lora_aug and fuse16 or ((i, "gu") not in lg and (i, "down") not in lg)))
            x2, x2w = self._norm_aug(h, L.ln2, lg.get((i, "gu")) if fused_gu and self.lora_aug else None, st, "t_gu")
            if fused_gu:
                gu = torch.empty((rows, 2 * I), **bf)                    # SwiGLU in the epilogue; gate | up kept as bf16 for the backward
                if not ops.gemm16_fragw_swiglu_train(0, x2w, tw[0], 2 * I, x2w.shape[1], act, gu):
                    if x2w is not x2:
                        raise RuntimeError("train_engine: the fused SwiGLU product declined the augmented gate|up shape")
                    gu = None
            if gu is None:
                gu = torch.empty((rows, 2 * I), **f32)
                ops.gemm16(x2, None, self._fwd_weight(L.wgu), None, 2 * I, ops.EPI_F32, c=gu)
                if (i, "gu") in lg and "t_gu" not in st:
                    st["t_gu"] = self._lora_fwd(lg[(i, "gu")], x2, gu)
                ops.swiglu_fwd(gu, act)
            h_out = torch.empty_like(h)
            ops.gemm16(act, None, self._fwd_weight(L.wdown), None, H, ops.EPI_RESID, c=h_out, resid=h)
            if (i, "down") in lg:
                st["t_down"] = self._lora_fwd(lg[(i, "down")], act, h_out)
            st.update(x2=x2, gu=gu, act=act, h_out=h_out)
            return st

        saved = []
        for i, L in enumerate(eng.layers):
            st = layer_forward(i, L, h)
            h = st.pop("h_out")
            saved.append({"h_in": st["h_in"]} if self.gradient_checkpointing else st)
            del st
        xf = torch.empty((rows, H), **bf)
        ops.rmsnorm_bf16(h, eng.norm, d.rms_norm_eps, xf)
        logits = torch.empty((rows, V), **f32)
        ops.gemm16(xf, None, eng.lm_head, None, V, ops.EPI_F32, c=logits)
        Vp = ops.round_up(V, 64)
        dlogits = torch.empty((rows, Vp), **bf)
        if pk is not None:
            # per micro-batch: the mean over ITS shifted targets.  Every sequence's first label is -100, so no row predicts across a
            # boundary; a group's last row is the last position of its (1, rows) call and does not count either.
            lab, loss = labels.reshape(-1).to(dev), None
            for (r0, r1) in pk.groups:
                li = ops.cross_entropy_fwd_bwd(logits[r0:r1].view(1, r1 - r0, V), lab[r0:r1].view(1, r1 - r0), dlogits[r0:r1], loss_scale)
                loss = li if loss is None else loss + li
            loss = loss / len(pk.groups)
        elif loss_groups > 1:
            assert B % loss_groups == 0, "loss_groups must divide the batch"
            gb, lab = B // loss_groups, labels.to(dev)
            lg = logits.view(B, S, V)
            loss = None
            for gi in range(loss_groups):
                li = ops.cross_entropy_fwd_bwd(lg[gi * gb: (gi + 1) * gb], lab[gi * gb: (gi + 1) * gb], dlogits[gi * gb * S: (gi + 1) * gb * S], loss_scale)
                loss = li if loss is None else loss + li
            loss = loss / loss_groups
        else:
            loss = ops.cross_entropy_fwd_bwd(logits.view(B, S, V), labels.to(dev), dlogits, loss_scale)
        del logits
        # ---------------- backward ----------------
        if ev is not None:
            ev[1].record()
        g = self.grads
        lg, frozen = self._lora_groups, self.frozen
        dtmp = torch.empty((rows, H), **f32)
        self._dx(dlogits, eng.lm_head, dtmp)                           # d(norm output); lm_head itself is frozen
        dh = torch.empty((rows, H), **f32)
        # augmented K: dh16 is the head of a [rows][H + rp] buffer whose tail takes dT = dh (s B) of down_proj / o_proj
        aug_bwd = self.lora_aug and fuse16 and fused_rows and bool(lg)
        dh16w = torch.empty((rows, H + (self.lora.rp if aug_bwd else 0)), **bf) if fuse16 else None
        dh16 = dh16w[:, :H] if fuse16 else None
        ops.rmsnorm_bwd(h, eng.norm, dtmp, d.rms_norm_eps, dh, False, self._ln_sink if frozen else g["norm"], dx16=dh16)
        del dlogits
        Sp = ops.round_up(S, 64)
        BH = B * nh
        scale = 1.0 / math.sqrt(hd)
        for i in reversed(range(len(eng.layers))):
            L, st = eng.layers[i], saved[i]
            if self.gradient_checkpointing:          # recompute this layer's forward from its saved input (K / V caches included)
                st = layer_forward(i, L, st["h_in"])
                st.pop("h_out")
                saved[i] = None
            pre = f"layers.{i}."
            # ---- MLP ----
            if not fuse16:
                dh16, _ = ops.split16(dh, _BF, want_lo=False, kmult=64)
                dh16 = dh16[:, :H]
            dgu = torch.empty((rows, 2 * I), **bf)
            tw = self.twins.get(pre + "wdown")
            gd = lg.get((i, "down")) if aug_bwd and tw is not None and st["gu"].dtype == _BF else None
            a_in = dh16
            if gd is not None:                                           # [dh | dT] . [W^T | A^T]^T: the adapter's share of d(act) inside the product
                a_in = dh16w
                ops.lora_down(dh16, gd.sb_t, dh16w[:, H:], k=H)
                self._lora_bwd(gd, dh16, st["act"], st["t_down"], None, dt=dh16w[:, H:])
            if not (st["gu"].dtype == _BF and tw is not None and
                    ops.gemm16_fragw_swiglu_train(1, a_in, tw[1], I, a_in.shape[1], dgu, st["gu"])):   # d(act) never leaves the accumulators
                dact = torch.empty((rows, I), **f32)
                self._dx(dh16, L.wdown, dact)
                if gd is not None:
                    raise RuntimeError("train_engine: the fused SwiGLU backward declined the augmented down_proj shape")
                if (i, "down") in lg:
                    self._lora_bwd(lg[(i, "down")], dh16, st["act"], st["t_down"], dact)
                if st["gu"].dtype == _BF:
                    raise RuntimeError("train_engine: bf16 gate|up was saved but the fused SwiGLU backward declined the shape")
                ops.swiglu_bwd(st["gu"], dact, dgu)
                del dact
            if not frozen:
                self._dw(dh16, st["act"], g[pre + "wdown"], pre + "wdown")
            self._dx(dgu, L.wgu, dtmp)
            if (i, "gu") in lg:
                self._lora_bwd(lg[(i, "gu")], dgu, st["x2"], st["t_gu"], dtmp)
            if not frozen:
                self._dw(dgu, st["x2"], g[pre + "wgu"], pre + "wgu")
            del dgu
            ops.rmsnorm_bwd(st["h_mid"], L.ln2, dtmp, d.rms_norm_eps, dh, True, self._ln_sink if frozen else g[pre + "ln2"], dx16=dh16)
            # ---- attention ----
            if not fuse16:
                dh16, _ = ops.split16(dh, _BF, want_lo=False, kmult=64)
                dh16 = dh16[:, :H]
            q = st["q"].view(BH, S, hd)
            kc, vtc = caches(i)
            # flash-style backward (csrc/attn_bwd.hip): P is recomputed per tile from the forward's log-sum-exp, no S x S matrix
            # exists and no operand is transposed
            v_rm = st.get("v_rm")
            if v_rm is None:                                             # (V back to row-major from the transposed cache)
                v_rm = torch.empty((BH, S, hd), **bf)
                ops.transpose16(vtc, smax, hd, S, v_rm, hd, BH, hd * smax, S * hd)
            dsum = torch.empty((BH, S), **f32)
            dqkv = torch.empty((rows, 3 * H), **bf)
            tw = self.twins.get(pre + "wo")
            go = lg.get((i, "o"))
            if self.attn_glue_fused and tw is not None and fused_rows and hd == 128 and (go is None or aug_bwd):
                # round 6: d(att) leaves the o_proj dX product as bf16, token-major, and is read like that by the attention backward, whose
                # epilogues write d(q | k | v) with the RoPE backward applied: no fp32 d(att), split16, split_heads16, fp32 dq / dk / dv
                # or rope_merge_bwd passes
                datt16 = torch.empty((rows, H), **bf)
                if go is not None:                                          # [dh | dT] . [Wo^T | Ao^T]^T
                    ops.lora_down(dh16, go.sb_t, dh16w[:, H:], k=H)
                    self._lora_bwd(go, dh16, st["att"], st["t_o"], None, dt=dh16w[:, H:])
                    ops.gemm16_fragw(dh16w, None, tw[1], None, H, dh16w.shape[1], ops.EPI_OUT16, out_hi=datt16)
                elif dh16.is_contiguous():
                    ops.gemm16_fragw(dh16, None, tw[1], None, H, H, ops.EPI_OUT16, out_hi=datt16)
                else:
                    ops.gemm16_fragw(dh16w, None, tw[1], None, H, H, ops.EPI_OUT16, out_hi=datt16)
                if not frozen:
                    self._dw(dh16, st["att"], g[pre + "wo"], pre + "wo")
                if pk is None:
                    ops.attn_backward_fused(q, kc, v_rm, datt16, st["att"], st["lse"], dsum, B, S, nh, hd, eng.cos, eng.sin, 0, dqkv)
                else:                                                       # (the engine's own tables: the kernel rotates by the position inside the sequence)
                    ops.attn_backward_fused_varlen(q, kc, v_rm, datt16, st["att"], st["lse"], dsum, pk.table, pk.seqs, pk.max_len, S, nh, hd,
                                                   eng.cos, eng.sin, dqkv)
            else:
                self._dx(dh16, L.wo, dtmp)                                  # d(att)
                if (i, "o") in lg:
                    self._lora_bwd(lg[(i, "o")], dh16, st["att"], st["t_o"], dtmp)
                if not frozen:
                    self._dw(dh16, st["att"], g[pre + "wo"], pre + "wo")
                datt16, _ = ops.split16(dtmp, _BF, want_lo=False, kmult=64)
                dO = torch.empty((BH, S, hd), **bf)
                ops.split_heads16(datt16[:, :H].contiguous() if datt16.shape[1] != H else datt16, B, S, nh, hd, dO)
                dq = torch.empty((BH, S, hd), **f32)
                dk = torch.empty((BH, S, hd), **f32)
                dv = torch.empty((BH, S, hd), **f32)
                if pk is None:
                    ops.attn_backward(q, kc, v_rm, dO, st["att"], st["lse"], dsum, B, S, nh, hd, dq, dk, dv)
                else:
                    ops.attn_backward_varlen(q, kc, v_rm, dO, st["att"], st["lse"], dsum, pk.table, pk.seqs, pk.max_len, S, nh, hd, dq, dk, dv)
                ops.rope_merge_bwd(dq, dk, dv, cos, sin, B, S, nh, hd, 0, dqkv)
            self._dx(dqkv, L.wqkv, dtmp)
            if (i, "qkv") in lg:
                self._lora_bwd(lg[(i, "qkv")], dqkv, st["x1"], st["t_qkv"], dtmp)
            if not frozen:
                self._dw(dqkv, st["x1"], g[pre + "wqkv"], pre + "wqkv")
            ops.rmsnorm_bwd(st["h_in"], L.ln1, dtmp, d.rms_norm_eps, dh, True, self._ln_sink if frozen else g[pre + "ln1"], dx16=dh16)
            saved[i] = None
            if overlap_allreduce_world > 1 and (not frozen or lg):
                self._start_layer_allreduce(i)
        # ---- bottom: projector and the trainable embedding rows ----
        if seg_rows:
            ridx = torch.cat(seg_rows)
            dya = torch.empty((ridx.numel(), H), **f32)
            ops.gather_rows(dh, ridx, dya)
            ops.colsum_add(dya, g["proj_b"])
            dya16, _ = ops.split16(dya, _BF, want_lo=False, kmult=64)
            self._dw(dya16[:, :H], torch.cat(seg_a16, dim=0).contiguous(), g["proj_w"], "proj_w")
        if self.train_embed_all:
            keep = torch.ones((rows,), dtype=torch.bool, device=dev)
            if seg_rows:
                keep[torch.cat(seg_rows)] = False
        elif self.embed_grad_tokens:
            keep = torch.isin(ids_flat, torch.tensor(sorted(self.embed_grad_tokens), dtype=ids_flat.dtype, device=dev))
        else:
            keep = None
        if keep is not None:
            ridx = keep.nonzero().reshape(-1)
            if ridx.numel():
                tmp = torch.empty((ridx.numel(), H), **f32)
                ops.gather_rows(dh, ridx, tmp)
                ops.scatter_add_rows(tmp, ids_flat[ridx].contiguous(), g["embed"])
        self._norm_collect = False
        self.micro_batches += 1
        if ev is not None:
            ev[2].record()
            self.phase_events = ev                      # of the LAST call: bench.py reads forward / backward ms of a micro-batch
        return loss

    # ------------------------------------------------------------------------------------------
    def _layer_span(self, i: int) -> Tuple[int, int]:
        """[start, end) of decoder layer i inside the flat gradient (its six tensors are contiguous)."""
        if getattr(self, "frozen", False):               # the layer's adapter factors (contiguous; every layer has the same targets)
            names = [n for n, _ in self.params if n.startswith(f"layers.{i}.")]
            o0, _ = self._slices[names[0]]
            o1, n1 = self._slices[names[-1]]
            return o0, o1 + n1
        o0, _ = self._slices[f"layers.{i}.wqkv"]
        o1, n1 = self._slices[f"layers.{i}.ln2"]
        return o0, o1 + n1

    def _start_layer_allreduce(self, i: int) -> None:
        from .. import dist as D

        o0, o1 = self._layer_span(i)
        if not hasattr(self, "_inflight"):
            self._inflight, self._reduced = [], []
        self._inflight.append(D.all_reduce_sum_async(self.flat_grad[o0:o1], getattr(self, "grad_comm", torch.float32), self._stage(o0, o1)))
        self._reduced.append((o0, o1))

    def _stage(self, o0: int, o1: int):
        """Slice [o0, o1) of the persistent reduced-precision transport buffer (allocated once, on the first exchange that needs
        it: 2 bytes per gradient element, 13.5 GB at 7B); None when the gradients travel as fp32."""
        comm = getattr(self, "grad_comm", torch.float32)
        if comm == torch.float32:
            return None
        st = getattr(self, "_flat_stage", None)
        if st is None or st.dtype != comm or st.numel() != self.flat_grad.numel():
            st = torch.empty(self.flat_grad.numel(), dtype=comm, device=self.flat_grad.device)
            self._flat_stage = st
        return st[o0:o1]

    def _finalize_grads(self) -> None:
        """A matrix whose dW product never ran since zero_grad() (e.g. mm_projector on a text-only batch) still holds the
        previous step's values: zero it before anyone reads the gradients."""
        for name in getattr(self, "_fresh", ()):
            self.grads[name].zero_()
        self._fresh = set()

    def allreduce_grads(self, world: int, bucket_elems: int = 64 * 1024 * 1024) -> None:
        """Sum gradients over the data-parallel ranks (RCCL on GPUs): large flat buckets; the division by the world
        size is folded into the optimizer's grad_scale.  Slices already exchanged during the backward
        (``overlap_allreduce_world``) are skipped; everything in flight is waited for."""
        self._finalize_grads()
        done = sorted(getattr(self, "_reduced", []))
        works = list(getattr(self, "_inflight", []))
        self._inflight, self._reduced = [], []
        timed = getattr(self, "time_exchange", False) and self.flat_grad.is_cuda
        if timed:                                        # everything between these two events is exchange the backward did not hide
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        if world > 1:
            from .. import dist as D

            self._norm_spans = []                        # the exchange changes every gradient: sums of squares taken before it are stale
            comm = getattr(self, "grad_comm", torch.float32)
            n = self.flat_grad.numel()
            pos = 0
            for a, b in done + [(n, n)]:                  # the gaps between the spans reduced so far
                for o in range(pos, a, bucket_elems):
                    e = min(o + bucket_elems, a)
                    works.append(D.all_reduce_sum_async(self.flat_grad[o:e], comm, self._stage(o, e)))
                pos = max(pos, b)
        for w in works:
            w.wait()
        if timed:
            ev1.record()
            self._exchange_events = getattr(self, "_exchange_events", []) + [(ev0, ev1)]

    def exposed_exchange_ms(self) -> float:
        """Sum over the steps since the last call of the compute-stream time spent in allreduce_grads() -- the part of the
        gradient exchange the backward did not overlap (0 on one GPU).  Needs ``time_exchange = True``."""
        evs, self._exchange_events = self._exchange_events, []
        if not evs:
            return 0.0
        torch.cuda.synchronize()
        return float(sum(a.elapsed_time(b) for a, b in evs))

    def _grad_sumsq(self) -> torch.Tensor:
        """Device double: sum of g^2 over the whole flat gradient (the slices whose dW product already added its share,
        ``last_micro_batch``, are not read again).  Call after ``allreduce_grads``."""
        self._finalize_grads()
        spans = sorted(self._norm_spans)
        if spans:
            acc, first = self._norm_acc, False
        else:
            acc, first = torch.empty((1,), dtype=torch.float64, device=self.flat_grad.device), True
        pos, n = 0, self.flat_grad.numel()
        for a, b in spans + [(n, n)]:                       # the gaps between the spans summed so far
            if a > pos:
                ops.sumsq_f32(self.flat_grad[pos:a], out=acc, accumulate=not first)
                first = False
            pos = max(pos, b)
        self._norm_spans = []
        return acc

    def grad_norm(self, world: int = 1) -> float:
        """L2 norm of the (rank-averaged) gradient over every trainable tensor -- what torch.nn.utils.clip_grad_norm_ returns in HF
        Trainer's step (a host read of the device scalar)."""
        return math.sqrt(float(self._grad_sumsq().item())) / world

    @property
    def last_grad_norm(self) -> Optional[float]:
        """Gradient norm of the last ``step(max_grad_norm=...)`` (read from the device on first access), else None."""
        ss = self._last_sumsq
        if ss is None:
            return None
        if isinstance(ss, tuple):
            self._last_sumsq = math.sqrt(float(ss[0].item())) / ss[1]
        return self._last_sumsq

    def step(self, world: int = 1, max_grad_norm: Optional[float] = None) -> None:
        """AdamW over every trainable tensor (bias-corrected, decoupled weight decay), then zero the gradients.
        ``max_grad_norm``: HF Trainer's gradient clipping (``TrainingArguments.max_grad_norm``, default 1.0, which the reference's
        train_llark.sh leaves alone): gradients are scaled by min(1, max_grad_norm / (norm + 1e-6)).  The squared norm stays in
        device memory and the coefficient is formed inside the AdamW kernels (``llark_adamw_clip``): no host read between the
        backward and the update, no extra pass over the gradients; ``last_grad_norm`` reads it back on demand."""
        if self.flat_m is None:
            raise RuntimeError("this HipLlamaTrainer was built with optimizer_state=False (autograd bridge): use a torch optimizer")
        self._finalize_grads()
        clip = max_grad_norm is not None and max_grad_norm > 0
        sumsq = None
        self._last_sumsq = None
        if clip:
            sumsq = self._grad_sumsq()
            self._last_sumsq = (sumsq.clone(), world)
        else:
            self._norm_spans = []                           # partial sums nobody asked for
        self.step_count += 1
        b1, b2 = self.betas
        n_lora = self.lora_flat.numel() if self.lora_flat is not None else 0
        if n_lora:                                          # every adapter master in one launch (flat fp32, the head of the table)
            ops.adamw(self.lora_flat, self.flat_grad[:n_lora], self.flat_m[:n_lora], self.flat_v[:n_lora], self.lr, b1, b2, self.eps,
                      self.wd, self.step_count, 1.0 / world, grad_sumsq=sumsq, max_grad_norm=float(max_grad_norm) if clip else 0.0)
            self._refresh_lora()
        for name, p in self.params:
            off, n = self._slices[name]
            if off < n_lora:
                continue
            tw = self.twins.get(name)
            if tw is not None:
                ops.adamw_twins(p, self.flat_grad[off: off + n], self.flat_m[off: off + n], self.flat_v[off: off + n], self.lr, b1, b2,
                                self.eps, self.wd, self.step_count, 1.0 / world, grad_sumsq=sumsq,
                                max_grad_norm=float(max_grad_norm) if clip else 0.0, wfrag=tw[0], rope_rows=tw[2], wtfrag=tw[1])
                continue
            ops.adamw(p.view(-1), self.flat_grad[off: off + n], self.flat_m[off: off + n], self.flat_v[off: off + n],
                      self.lr, b1, b2, self.eps, 0.0 if p.dim() == 1 else self.wd, self.step_count, 1.0 / world,
                      grad_sumsq=sumsq, max_grad_norm=float(max_grad_norm) if clip else 0.0)
        self._weights_changed()
        self.zero_grad()

    # ------------------------------------------------------------------------------------------
    def export_grads_hf(self) -> Dict[str, torch.Tensor]:
        """Gradients under the reference's state-dict names / layouts (for parity tests and checkpoint tooling)."""
        self._finalize_grads()
        d = self.eng.dims
        H, I = d.hidden_size, d.intermediate_size
        out = {}
        if self.frozen:                                     # adapter gradients under the peft names; nothing for a frozen tensor
            out.update(self._adapters_from(self.grads))
            out["model.embed_tokens.weight"] = self.grads["embed"]
            if "proj_w" in self.grads:
                out["model.mm_projector.weight"] = self.grads["proj_w"]
                out["model.mm_projector.bias"] = self.grads["proj_b"]
            return out
        for i in range(d.num_hidden_layers):
            p = f"model.layers.{i}"
            gq = self.grads[f"layers.{i}.wqkv"]
            out[f"{p}.self_attn.q_proj.weight"], out[f"{p}.self_attn.k_proj.weight"], out[f"{p}.self_attn.v_proj.weight"] = (
                gq[:H], gq[H: 2 * H], gq[2 * H:])
            out[f"{p}.self_attn.o_proj.weight"] = self.grads[f"layers.{i}.wo"]
            gg = self.grads[f"layers.{i}.wgu"].view(I // 32, 2, 32, H)
            out[f"{p}.mlp.gate_proj.weight"] = gg[:, 0].reshape(I, H)
            out[f"{p}.mlp.up_proj.weight"] = gg[:, 1].reshape(I, H)
            out[f"{p}.mlp.down_proj.weight"] = self.grads[f"layers.{i}.wdown"]
            out[f"{p}.input_layernorm.weight"] = self.grads[f"layers.{i}.ln1"]
            out[f"{p}.post_attention_layernorm.weight"] = self.grads[f"layers.{i}.ln2"]
        out["model.norm.weight"] = self.grads["norm"]
        out["model.embed_tokens.weight"] = self.grads["embed"]
        if "proj_w" in self.grads:
            out["model.mm_projector.weight"] = self.grads["proj_w"]
            out["model.mm_projector.bias"] = self.grads["proj_b"]
        return out
