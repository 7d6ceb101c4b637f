"""LoRA adapters served per request: PEFT adapter directories -> the device layout of ops.lora_add.

`LORA_ADAPTERS=name=dir[,name=dir...]` (at most 8) names PEFT directories (`adapter_config.json` +
`adapter_model.safetensors`).  Every adapter is packed, per layer and per fused weight of models/weights.py, into

  A     bf16 [n_adapters, S, R, K]   lora_A of the S sub-modules stacked in the fused weight, rows >= r zero
  B     bf16 [n_adapters, N, R]      lora_B of those sub-modules, stacked as the fused weight stacks them
  scale fp32 [n_adapters, S]         alpha / r (alpha / sqrt(r) with rslora); 0 = the adapter has no such module
  seg   S + 1 boundaries of N

with wqkv S = 3 (q | k | v), wo S = 1, w13 S = 2 (gate | up), w2 S = 1 and R = MAX_LORA_RANK (16, 32 or 64).
The fused layouts keep HF's row order (the loader applies no q / k permutation), so lora_B rows go in as they are.

Supported PEFT subset: plain LoRA (optionally rslora) on the seven projections of a dense Llama, TP = 1.  Anything
else is refused when the engine is built, with a message that names the adapter and the reason.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .config import ModelConfig

MAX_ADAPTERS = 8
RANKS = (16, 32, 64)
# PEFT module -> (fused weight, segment)
MODULES = {"q_proj": ("wqkv", 0), "k_proj": ("wqkv", 1), "v_proj": ("wqkv", 2), "o_proj": ("wo", 0),
           "gate_proj": ("w13", 0), "up_proj": ("w13", 1), "down_proj": ("w2", 0)}
FUSED = ("wqkv", "wo", "w13", "w2")
_KEY = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])\.weight$")


class LoraError(ValueError):
    """An adapter (or the adapter configuration) the engine does not serve."""


def parse_adapters(spec: str) -> List[Tuple[str, str]]:
    """`name=dir[,name=dir...]` -> [(name, dir)] in slot order."""
    out: List[Tuple[str, str]] = []
    for part in (p.strip() for p in (spec or "").split(",")):
        if not part:
            continue
        name, eq, path = part.partition("=")
        name, path = name.strip(), path.strip()
        if not eq or not name or not path:
            raise LoraError(f"LORA_ADAPTERS: {part!r} is not name=dir")
        if any(n == name for n, _ in out):
            raise LoraError(f"LORA_ADAPTERS: adapter {name!r} is named twice")
        out.append((name, path))
    if len(out) > MAX_ADAPTERS:
        raise LoraError(f"LORA_ADAPTERS: {len(out)} adapters, at most {MAX_ADAPTERS} are served")
    return out


def kubectl_slot(settings) -> Optional[int]:
    """LORA_KUBECTL -> its slot among LORA_ADAPTERS (None: unset); an unknown name raises LoraError."""
    name = getattr(settings, "LORA_KUBECTL", "") or ""
    if not name:
        return None
    names = [n for n, _ in parse_adapters(getattr(settings, "LORA_ADAPTERS", ""))]
    if name not in names:
        raise LoraError(f"LORA_KUBECTL={name!r} is not one of LORA_ADAPTERS ({', '.join(names) or 'none configured'})")
    return names.index(name)


def module_shapes(cfg: ModelConfig) -> Dict[str, Tuple[int, int]]:
    """PEFT module -> (out, in) of the base projection."""
    H, I = cfg.hidden, cfg.intermediate
    return {"q_proj": (cfg.q_size, H), "k_proj": (cfg.kv_size, H), "v_proj": (cfg.kv_size, H),
            "o_proj": (H, cfg.q_size), "gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I)}


def fused_segments(cfg: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Fused weight -> boundaries of its stacked sub-modules."""
    q, kv, I, H = cfg.q_size, cfg.kv_size, cfg.intermediate, cfg.hidden
    return {"wqkv": (0, q, q + kv, q + 2 * kv), "wo": (0, H), "w13": (0, I, 2 * I), "w2": (0, H)}


@dataclass
class Adapter:
    name: str
    r: int
    scale: float
    tensors: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]]   # (layer, module) -> (A [r, in], B [out, r])


def read_adapter(name: str, path: str, cfg: ModelConfig, max_rank: int) -> Adapter:
    """Read and check one PEFT directory."""
    def refuse(why: str):
        raise LoraError(f"LoRA adapter {name!r} ({path}): {why}")

    cfg_path = os.path.join(path, "adapter_config.json")
    st_path = os.path.join(path, "adapter_model.safetensors")
    if not os.path.isfile(cfg_path) or not os.path.isfile(st_path):
        refuse("adapter_config.json and adapter_model.safetensors are needed")
    with open(cfg_path) as f:
        ac = json.load(f)
    if ac.get("peft_type", "LORA") != "LORA":
        refuse(f"peft_type {ac.get('peft_type')!r} is not LORA")
    if ac.get("use_dora"):
        refuse("DoRA (use_dora) is not supported")
    if ac.get("bias", "none") != "none":
        refuse(f"bias={ac.get('bias')!r}: only bias=\"none\" is supported")
    if ac.get("modules_to_save"):
        refuse(f"modules_to_save={ac.get('modules_to_save')!r} is not supported")
    r = int(ac.get("r", 0))
    if r < 1:
        refuse(f"r={r} is not a rank")
    if r > max_rank:
        refuse(f"r={r} is larger than MAX_LORA_RANK={max_rank}")
    targets = ac.get("target_modules") or []
    if isinstance(targets, str):
        targets = [targets]
    for t in targets:
        if t.split(".")[-1] not in MODULES:
            refuse(f"target module {t!r} is outside the seven projections {sorted(MODULES)}")
    alpha = float(ac.get("lora_alpha", r))
    scale = alpha / math.sqrt(r) if ac.get("use_rslora") else alpha / r
    from safetensors.torch import load_file
    raw = load_file(st_path)
    shapes = module_shapes(cfg)
    halves: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for key, t in raw.items():
        m = _KEY.match(key)
        if m is None or m.group(2) not in MODULES:
            refuse(f"tensor {key!r} is outside the seven projections' lora_A / lora_B weights")
        layer, mod, half = int(m.group(1)), m.group(2), m.group(3)
        if layer >= cfg.num_layers:
            refuse(f"tensor {key!r}: {cfg.name} has {cfg.num_layers} layers")
        out_f, in_f = shapes[mod]
        want = (r, in_f) if half == "A" else (out_f, r)
        if tuple(t.shape) != want:
            refuse(f"tensor {key!r} has shape {tuple(t.shape)}, {cfg.name} needs {want}")
        halves.setdefault((layer, mod), {})[half] = t
    tensors = {}
    for (layer, mod), ab in halves.items():
        if set(ab) != {"A", "B"}:
            refuse(f"layer {layer} {mod}: lora_A and lora_B come together")
        tensors[(layer, mod)] = (ab["A"], ab["B"])
    if not tensors:
        refuse("no lora_A / lora_B tensors")
    return Adapter(name=name, r=r, scale=scale, tensors=tensors)


@dataclass
class FusedLora:
    """One fused weight's adapters in ops.lora_add's layout."""
    A: torch.Tensor
    B: torch.Tensor
    scale: torch.Tensor
    seg: Tuple[int, ...]


class LoraSet:
    """The adapters resident on one engine: names in slot order and, per layer, fused weight -> FusedLora."""

    def __init__(self, names: List[str], rank: int, layers: List[Dict[str, FusedLora]]):
        self.names = list(names)
        self.rank = rank
        self.layers = layers

    def __len__(self) -> int:
        return len(self.names)

    def index(self, name: Optional[str]) -> Optional[int]:
        return self.names.index(name) if name in self.names else None


def pack_adapters(adapters: List[Adapter], cfg: ModelConfig, max_rank: int, device="cpu",
                  dtype=torch.bfloat16) -> LoraSet:
    n, R = len(adapters), max_rank
    shapes, segs = module_shapes(cfg), fused_segments(cfg)
    layers = []
    for li in range(cfg.num_layers):
        fused = {}
        for w in FUSED:
            mods = sorted((s, m) for m, (fw, s) in MODULES.items() if fw == w)
            seg = segs[w]
            K = shapes[mods[0][1]][1]
            A = torch.zeros((n, len(mods), R, K), dtype=dtype)
            B = torch.zeros((n, seg[-1], R), dtype=dtype)
            scale = torch.zeros((n, len(mods)), dtype=torch.float32)
            for ai, ad in enumerate(adapters):
                for s, m in mods:
                    ab = ad.tensors.get((li, m))
                    if ab is None:
                        continue
                    A[ai, s, :ad.r] = ab[0].to(dtype)
                    B[ai, seg[s]:seg[s + 1], :ad.r] = ab[1].to(dtype)
                    scale[ai, s] = ad.scale
            fused[w] = FusedLora(A.to(device), B.to(device), scale.to(device), seg)
        layers.append(fused)
    return LoraSet([a.name for a in adapters], R, layers)


def load_adapters(spec: str, cfg: ModelConfig, max_rank: int = 16, device="cpu", tp_size: int = 1,
                  dtype=torch.bfloat16) -> Optional[LoraSet]:
    """LORA_ADAPTERS -> LoraSet (None when nothing is configured); raises LoraError for what is not served."""
    pairs = parse_adapters(spec)
    if not pairs:
        return None
    if max_rank not in RANKS:
        raise LoraError(f"MAX_LORA_RANK={max_rank}: choose from {RANKS}")
    names = ", ".join(n for n, _ in pairs)
    if cfg.is_moe:
        raise LoraError(f"LoRA adapters ({names}): {cfg.name} is a MoE model, adapters are served on dense models only")
    if tp_size > 1:
        raise LoraError(f"LoRA adapters ({names}): TP={tp_size}, adapters are served at TP=1 only")
    if cfg.vocab_size >= 1 << 20:
        raise LoraError(f"LoRA adapters ({names}): the prefix cache's adapter tag needs vocab_size < 2**20")
    adapters = [read_adapter(n, p, cfg, max_rank) for n, p in pairs]
    return pack_adapters(adapters, cfg, max_rank, device, dtype)
