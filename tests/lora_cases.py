"""Case builders shared by tests/test_lora_cpu.py and tests/test_lora_gpu.py (ops.lora_add, models/lora.py).

Exact probes: x, A and B hold -1, 0, 1, so t = x A^T is an integer of magnitude <= K <= 256 (exact in bf16);
y holds small integers and every scale is a power of two, so each fp32 value on the way is exact and the kernel
must equal the reference bit for bit.  The shapes straddle the kernel's own geometry (TILE_ROWS, TILE_N: asserted
against the library's exports by the GPU test).
"""
import json
import math
import os

import torch

from ai_agent_kubectl_amd.models import lora as mlora

BF = torch.bfloat16
TILE_ROWS = 16    # csrc/lora.hip LORA_ROWS
TILE_N = 256      # csrc/lora.hip LORA_TN
SENTINEL = 0x7FA5   # a NaN pattern no arithmetic here produces: rows of -1 must keep it

EXACT_T = (1, 3, 16, 17, 33, 2 * TILE_ROWS + TILE_ROWS + 1)
EXACT_K = (64, 192)
EXACT_SEGS = ((16, 16, 16), (48, 16, 32), (TILE_N + 16,), (32, TILE_N + 16))
EXACT_RANKS = ((16, 8), (64, 64))   # (padded R, the adapters' own r)
EXACT_CASES = [(T, K, segs, R, r) for segs in EXACT_SEGS for R, r in EXACT_RANKS for K in EXACT_K for T in EXACT_T]


def boundaries(widths):
    seg = [0]
    for w in widths:
        seg.append(seg[-1] + w)
    return tuple(seg)


def row_pattern(T, n_adapters, seed=0):
    """Adapters interleaved with -1 inside every 16-row tile, in no order, the last slot used (also at T = 1)."""
    base = [n_adapters - 1, -1, 0, 1 % n_adapters, -1, n_adapters - 1, 0, 0, -1, 1 % n_adapters]
    return torch.tensor([base[(i + seed) % len(base)] if i else n_adapters - 1 for i in range(T)], dtype=torch.int32)


def exact_case(T, K, widths, R, r, n_adapters=3, seed=0):
    """dict(y, x, row_adapter, A, B, scale, seg) on the CPU; adapter 1's first segment has scale 0."""
    g = torch.Generator().manual_seed(1000 * T + K + 7 * len(widths) + R + seed)
    seg = boundaries(widths)
    S, N = len(widths), seg[-1]

    def tri(shape):
        return (torch.randint(0, 3, shape, generator=g) - 1).to(BF)

    A = tri((n_adapters, S, R, K))
    B = tri((n_adapters, N, R))
    A[:, :, r:] = 0          # an adapter of rank r < R is zero beyond r
    B[:, :, r:] = 0
    x = tri((T, K))
    y = (torch.randint(0, 17, (T, N), generator=g) - 8).to(BF)
    ra = row_pattern(T, n_adapters, seed)
    y.view(torch.int16)[ra < 0] = SENTINEL
    scale = torch.tensor([[2.0 ** ((a + s) % 4 - 1) for s in range(S)] for a in range(n_adapters)])
    scale[1 % n_adapters, 0] = 0.0
    return dict(y=y, x=x, row_adapter=ra, A=A, B=B, scale=scale, seg=seg)


def real_case(T, K, widths, R=16, n_adapters=2, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed + T + K)
    seg = boundaries(widths)
    S, N = len(widths), seg[-1]
    A = (torch.randn((n_adapters, S, R, K), generator=g) * 0.05).to(BF)
    B = (torch.randn((n_adapters, N, R), generator=g) * 0.05).to(BF)
    x = torch.randn((T, K), generator=g).to(BF)
    y = torch.randn((T, N), generator=g).to(BF)
    ra = torch.tensor([(-1, 0, 1 % n_adapters, 0)[(i + 1) % 4] for i in range(T)], dtype=torch.int32)
    scale = torch.tensor([[2.0, 0.5, 1.25][:S] if a == 0 else [1.0, 3.0, 0.75][:S] for a in range(n_adapters)])
    c = dict(y=y, x=x, row_adapter=ra, A=A, B=B, scale=scale, seg=seg)
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def float64_truth(c):
    """(y_ref float64 [T, N], bound float64 [T, N]) of a case: the unrounded result and the issue's per-element
    bound scale * sum_j |B[n, j]| (|t_j| 2^-8 + K 2^-23 sum_k |x_k A_jk|) + |y_ref| 2^-8 (one bf16 ulp of t, fp32
    accumulation, one bf16 ulp of y); rows of -1 and segments of scale 0: y itself, bound 0."""
    y, x, ra, A, B, scale, seg = (c[k] for k in ("y", "x", "row_adapter", "A", "B", "scale", "seg"))
    K = x.shape[1]
    y_ref = y.double().clone()
    bound = torch.zeros_like(y_ref)
    x64 = x.double()
    for a in range(A.shape[0]):
        rows = (ra == a).nonzero().flatten()
        if rows.numel() == 0:
            continue
        for s in range(len(seg) - 1):
            sc = float(scale[a, s])
            if sc == 0.0:
                continue
            A64, B64 = A[a, s].double(), B[a, seg[s]:seg[s + 1]].double()
            t = x64[rows] @ A64.T
            tabs = x64[rows].abs() @ A64.abs().T
            yr = y_ref[rows, seg[s]:seg[s + 1]] + sc * (t @ B64.T)
            y_ref[rows, seg[s]:seg[s + 1]] = yr
            bound[rows, seg[s]:seg[s + 1]] = abs(sc) * ((t.abs() * 2.0 ** -8 + K * 2.0 ** -23 * tabs) @ B64.abs().T) \
                + yr.abs() * 2.0 ** -8
    return y_ref, bound


def rounded_truth(c):
    """The definition in float64 with t rounded to bf16 and y rounded once: what ops/reference.py must give up to
    fp32 accumulation (a bf16 tie aside)."""
    y, x, ra, A, B, scale, seg = (c[k] for k in ("y", "x", "row_adapter", "A", "B", "scale", "seg"))
    out = y.double().clone()
    for a in range(A.shape[0]):
        rows = (ra == a).nonzero().flatten()
        for s in range(len(seg) - 1):
            sc = float(scale[a, s])
            if sc == 0.0 or rows.numel() == 0:
                continue
            t = (x[rows].double() @ A[a, s].double().T).to(BF).double()
            out[rows, seg[s]:seg[s + 1]] += sc * (t @ B[a, seg[s]:seg[s + 1]].double().T)
    return out


# ---- PEFT directories ----------------------------------------------------------------------------------------
PEFT_PREFIX = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
               "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}


def peft_tensors(cfg, r, modules=tuple(mlora.MODULES), seed=0, std_a=0.05, std_b=0.05, zero_b=False):
    """{PEFT tensor name: fp32 tensor whose values are bf16 numbers} for every layer of cfg."""
    g = torch.Generator().manual_seed(seed)
    shapes = mlora.module_shapes(cfg)
    out = {}
    for li in range(cfg.num_layers):
        for m in modules:
            o, i = shapes[m]
            p = f"base_model.model.model.layers.{li}.{PEFT_PREFIX[m]}.{m}"
            out[p + ".lora_A.weight"] = (torch.randn((r, i), generator=g) * std_a).to(BF).float()
            b = torch.zeros((o, r)) if zero_b else torch.randn((o, r), generator=g) * std_b
            out[p + ".lora_B.weight"] = b.to(BF).float()
    return out


def write_peft_dir(path, tensors, r, alpha, modules=tuple(mlora.MODULES), **extra):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    cfg = {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "target_modules": list(modules), "bias": "none",
           "use_rslora": False, "use_dora": False, "modules_to_save": None}
    cfg.update(extra)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in tensors.items()}, os.path.join(path, "adapter_model.safetensors"))
    return str(path)


def merged_weights(W, cfg, tensors, scale):
    """The engine's weights with the adapter folded in, fp32: W + scale * B A per fused segment."""
    out = dict(W)
    segs = mlora.fused_segments(cfg)
    for li in range(cfg.num_layers):
        for m, (fw, s) in mlora.MODULES.items():
            p = f"base_model.model.model.layers.{li}.{PEFT_PREFIX[m]}.{m}"
            if p + ".lora_A.weight" not in tensors:
                continue
            key = f"layers.{li}.{fw}"
            if out[key] is W[key]:
                out[key] = W[key].float().clone()
            lo, hi = segs[fw][s], segs[fw][s + 1]
            delta = (tensors[p + ".lora_B.weight"].double() @ tensors[p + ".lora_A.weight"].double()).float()
            out[key][lo:hi] += scale * delta.to(out[key].device)
    return out


def lora_scale(r, alpha, rslora=False):
    return alpha / math.sqrt(r) if rslora else alpha / r
