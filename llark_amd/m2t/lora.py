"""LoRA adapters for the HIP training step: configuration, initialisation, peft key naming and the merge into a state dict.

Reference: ``m2t/train.py:82-99`` wraps the model with peft (``r=64``, ``lora_alpha=16``, every ``nn.Linear`` that
``find_all_linear_names`` returns minus ``lm_head``: q/k/v/o_proj, gate/up/down_proj) and saves the adapters with
``get_peft_state_maybe_zero_3`` plus ``non_lora_trainables.bin`` (``:264-273``).  For a target ``W [N][K]`` the layer computes
``y = W x + (alpha / r) B (A x)`` with ``A [r][K]`` (Kaiming-uniform, ``a = sqrt(5)``: nn.Linear's default) and ``B [N][r]`` (zero).

Kernel layout of one adapter pair (``HipLlamaTrainer``): fp32 masters ``A^T [K][rp]`` and ``B [N][rp]`` with the rank zero-padded to
``rp = round_up(r, 64)`` (the ``kp % 64 == 0`` rule of the GEMM kernels); padded columns are zero, take no gradient and no update.
``A`` is stored transposed so that both gradients, ``dB = s dY^T T`` and ``dA^T = x^T dT``, are the same token contraction
(``llark_lora_dw``).  Differences from peft: fp32 masters with bf16 operand copies; no dropout; no bias training.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import torch

TARGET_MODULES: Tuple[str, ...] = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
           "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
ADAPTER_WEIGHTS = "adapter_model.bin"
ADAPTER_CONFIG = "adapter_config.json"
NON_LORA_TRAINABLES = "non_lora_trainables.bin"
_PEFT_KEY = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\.(\w+)\.lora_([AB])\.weight$")


@dataclass
class LoraConfig:
    r: int = 64                                   # m2t/arguments.py lora_r
    alpha: float = 16.0                           # lora_alpha
    dropout: float = 0.0                          # the reference's default is 0.05; dropout is not built (check_supported_recipe)
    target_modules: Sequence[str] = field(default_factory=lambda: TARGET_MODULES)
    bias: str = "none"

    def __post_init__(self):
        self.target_modules = tuple(self.target_modules)
        if self.r <= 0 or self.r % 8 or self.r > 256:
            raise ValueError(f"lora r = {self.r}: the rank must be a multiple of 8 between 8 and 256")
        unknown = [m for m in self.target_modules if m not in TARGET_MODULES]
        if unknown or not self.target_modules:
            raise ValueError(f"lora target_modules {self.target_modules}: a non-empty subset of {TARGET_MODULES} is required")
        if self.dropout != 0.0:
            raise NotImplementedError(f"lora_dropout = {self.dropout}: adapter dropout is not implemented (use 0.0)")
        if self.bias != "none":
            raise NotImplementedError(f"lora_bias = {self.bias!r}: training biases with the adapters is not implemented (use 'none')")

    @property
    def rp(self) -> int:
        """The rank as the kernels see it: zero-padded to a multiple of 64."""
        return padded_rank(self.r)

    @property
    def scale(self) -> float:
        return float(self.alpha) / float(self.r)

    def to_peft_dict(self) -> dict:
        return {"peft_type": "LORA", "r": int(self.r), "lora_alpha": self.alpha, "target_modules": list(self.target_modules),
                "lora_dropout": float(self.dropout), "bias": self.bias, "task_type": "CAUSAL_LM"}

    @classmethod
    def from_peft_dict(cls, d: dict) -> "LoraConfig":
        return cls(r=int(d["r"]), alpha=float(d["lora_alpha"]), dropout=float(d.get("lora_dropout", 0.0)),
                   target_modules=tuple(d["target_modules"]), bias=d.get("bias", "none"))


def padded_rank(r: int) -> int:
    return (r + 63) // 64 * 64


def module_shape(module: str, hidden: int, intermediate: int) -> Tuple[int, int]:
    """(N, K) of the nn.Linear weight ``module`` wraps."""
    if module in ("gate_proj", "up_proj"):
        return intermediate, hidden
    if module == "down_proj":
        return hidden, intermediate
    return hidden, hidden


def peft_key(layer: int, module: str, which: str) -> str:
    """``base_model.model.model.layers.{i}.self_attn.q_proj.lora_A.weight`` (``which`` = 'A' or 'B')."""
    return f"base_model.model.model.layers.{layer}.{_PARENT[module]}.{module}.lora_{which}.weight"


def parse_peft_key(key: str) -> Optional[Tuple[int, str, str]]:
    """(layer, module, 'A' | 'B') of a peft adapter key, None for any other key."""
    m = _PEFT_KEY.match(key)
    if not m or m.group(3) not in _PARENT or _PARENT[m.group(3)] != m.group(2):
        return None
    return int(m.group(1)), m.group(3), m.group(4)


def hf_weight_key(layer: int, module: str) -> str:
    return f"model.layers.{layer}.{_PARENT[module]}.{module}.weight"


def init_adapters(cfg: LoraConfig, hidden: int, intermediate: int, num_layers: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """peft's initial state under peft names (fp32, CPU): ``lora_A`` Kaiming-uniform with a = sqrt(5) (bound 1 / sqrt(K)), ``lora_B`` zero.
    One seeded CPU generator, layers and modules in order: the same seed gives the same adapters on every rank."""
    gen = torch.Generator().manual_seed(int(seed))
    out = {}
    for i in range(num_layers):
        for mod in TARGET_MODULES:
            if mod not in cfg.target_modules:
                continue
            n, k = module_shape(mod, hidden, intermediate)
            bound = 1.0 / math.sqrt(k)
            out[peft_key(i, mod, "A")] = (torch.rand((cfg.r, k), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
            out[peft_key(i, mod, "B")] = torch.zeros((n, cfg.r), dtype=torch.float32)
    return out


def a_to_kernel(a: torch.Tensor, rp: int) -> torch.Tensor:
    """peft ``lora_A.weight`` [r][K] -> the master layout A^T [K][rp] (fp32, padded columns zero)."""
    r, k = a.shape
    out = torch.zeros((k, rp), dtype=torch.float32, device=a.device)
    out[:, :r] = a.float().t()
    return out


def b_to_kernel(b: torch.Tensor, rp: int) -> torch.Tensor:
    """peft ``lora_B.weight`` [N][r] -> B [N][rp] (fp32, padded columns zero)."""
    n, r = b.shape
    out = torch.zeros((n, rp), dtype=torch.float32, device=b.device)
    out[:, :r] = b.float()
    return out


def a_from_kernel(at: torch.Tensor, r: int) -> torch.Tensor:
    return at[:, :r].t().contiguous()


def b_from_kernel(b: torch.Tensor, r: int) -> torch.Tensor:
    return b[:, :r].contiguous()


def merge_into_state_dict(sd: Dict[str, torch.Tensor], adapters: Dict[str, torch.Tensor], cfg: LoraConfig) -> Dict[str, torch.Tensor]:
    """A copy of ``sd`` (HF names) with ``W + (alpha / r) B A`` in place of every adapted weight (peft's ``merge_and_unload``); the
    sum is formed in fp32 and stored in the weight's dtype.  Plain torch: this runs once per load, not on a hot path."""
    out = dict(sd)
    pairs: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for key, t in adapters.items():
        parsed = parse_peft_key(key)
        if parsed is None:
            raise KeyError(f"not a peft LoRA key: {key}")
        pairs.setdefault(parsed[:2], {})[parsed[2]] = t
    for (layer, mod), ab in sorted(pairs.items()):
        if "A" not in ab or "B" not in ab:
            raise KeyError(f"layer {layer} {mod}: lora_A and lora_B are both required")
        wk = hf_weight_key(layer, mod)
        if wk not in sd:
            raise KeyError(f"state dict lacks {wk}")
        w = sd[wk]
        a, b = ab["A"].to(w.device, torch.float32), ab["B"].to(w.device, torch.float32)
        if a.shape != (cfg.r, w.shape[1]) or b.shape != (w.shape[0], cfg.r):
            raise ValueError(f"layer {layer} {mod}: adapter shapes {tuple(a.shape)} / {tuple(b.shape)} do not fit {tuple(w.shape)} at r={cfg.r}")
        out[wk] = (w.float() + cfg.scale * (b @ a)).to(w.dtype)
    return out


def save_adapter(folder: str, adapters: Dict[str, torch.Tensor], cfg: LoraConfig) -> None:
    """``adapter_model.bin`` (peft names, unpadded rank) + ``adapter_config.json``."""
    os.makedirs(folder, exist_ok=True)
    torch.save({k: v.detach().cpu().contiguous() for k, v in adapters.items()}, os.path.join(folder, ADAPTER_WEIGHTS))
    with open(os.path.join(folder, ADAPTER_CONFIG), "w") as f:
        json.dump(cfg.to_peft_dict(), f, indent=2)


def load_adapter(folder: str) -> Tuple[Dict[str, torch.Tensor], LoraConfig]:
    with open(os.path.join(folder, ADAPTER_CONFIG)) as f:
        cfg = LoraConfig.from_peft_dict(json.load(f))
    adapters = torch.load(os.path.join(folder, ADAPTER_WEIGHTS), map_location="cpu")
    return adapters, cfg
