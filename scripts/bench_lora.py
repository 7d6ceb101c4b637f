"""Cost of serving LoRA adapters (Llama-3-8B, an r = 16 adapter on all seven projections): ops.lora_add per call at
the four projection shapes, and a decode step at batch 1, 16 and 256 with every row on the adapter, with half of
them, on the same eager plain route without adapter rows, and as the captured graph of a base-only batch (the path
an engine without adapters runs, which this feature leaves untouched)."""
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, SeqStatus, Sequence  # noqa: E402
from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM  # noqa: E402
from ai_agent_kubectl_amd.models import lora as mlora  # noqa: E402
from ai_agent_kubectl_amd.models.config import get_config  # noqa: E402

DEV = os.environ.get("MS_DEVICE", "cuda")
MODEL = os.environ.get("MS_MODEL", "llama3-8b")
BS = tuple(int(b) for b in os.environ.get("MS_BS", "1,16,256").split(",") if b)
OUT = os.environ.get("MS_OUT", os.path.join(ROOT, "profiles", "lora"))
RANK = 16
os.makedirs(OUT, exist_ok=True)
res = {}
if DEV == "cuda" and not torch.cuda.is_available():
    raise SystemExit("bench_lora.py measures on the GPU: no device found")


def save():
    with open(os.path.join(OUT, "bench_lora.json"), "w") as f:
        json.dump(res, f, indent=1)


def dev_time(fn, warm=5, reps=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # us


def write_adapter(path, cfg, seed=0):
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(seed)
    prefix = {m: ("self_attn" if fw in ("wqkv", "wo") else "mlp") for m, (fw, _) in mlora.MODULES.items()}
    t = {}
    for li in range(cfg.num_layers):
        for m, (o, i) in mlora.module_shapes(cfg).items():
            p = f"base_model.model.model.layers.{li}.{prefix[m]}.{m}"
            t[p + ".lora_A.weight"] = (torch.randn((RANK, i), generator=g) * 0.02).to(torch.bfloat16)
            t[p + ".lora_B.weight"] = (torch.randn((o, RANK), generator=g) * 0.02).to(torch.bfloat16)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": RANK, "lora_alpha": 2 * RANK, "target_modules": list(mlora.MODULES),
                   "bias": "none"}, f)
    save_file(t, os.path.join(path, "adapter_model.safetensors"))
    return path


cfg = get_config(MODEL)
segs = mlora.fused_segments(cfg)
shapes = mlora.module_shapes(cfg)
K_OF = {"wqkv": shapes["q_proj"][1], "wo": shapes["o_proj"][1], "w13": shapes["gate_proj"][1], "w2": shapes["down_proj"][1]}

# ---- the op: the four projection shapes, every row on one adapter / half of the rows on it ----
if DEV == "cuda":
    for T in BS:
        r = {}
        for w in mlora.FUSED:
            seg, K = segs[w], K_OF[w]
            S, N = len(seg) - 1, seg[-1]
            torch.manual_seed(T)
            x = torch.randn(T, K, device=DEV, dtype=torch.bfloat16)
            y = torch.randn(T, N, device=DEV, dtype=torch.bfloat16)
            A = (torch.randn(2, S, RANK, K, device=DEV) * 0.02).to(torch.bfloat16)
            B = (torch.randn(2, N, RANK, device=DEV) * 0.02).to(torch.bfloat16)
            sc = torch.full((2, S), 2.0, device=DEV)
            full = torch.zeros(T, dtype=torch.int32, device=DEV)
            half = torch.where(torch.arange(T, device=DEV) % 2 == 0, 0, -1).to(torch.int32)
            two = (torch.arange(T, device=DEV) % 2).to(torch.int32)
            for rnd in range(2):   # alternate, two rounds
                for name, ra in (("all", full), ("half", half), ("two_adapters", two)):
                    r.setdefault(f"{w}_{name}_us", []).append(
                        round(dev_time(lambda: ops.lora_add(y, x, ra, A, B, sc, seg)), 1))
            r[f"{w}_shape"] = dict(T=T, N=N, K=K, S=S, splits=int(ops.require().ka_lora_splits(T, S, K)))
        res[f"lora_add_T{T}"] = r
        print(T, r, flush=True)
    save()

# ---- the engine: a decode step at each batch ----
tmp = tempfile.mkdtemp(prefix="bench_lora_")
spec = "bench=" + write_adapter(os.path.join(tmp, "bench"), cfg)
eng = build_engine(EngineOptions(model=MODEL, device=DEV, max_batch=256, graph_buckets=(1, 2, 16, 256),
                                 kv_cache_tokens=49152, max_model_len=1024, max_batched_tokens=16384, use_graphs=True,
                                 lora_adapters=spec, max_lora_rank=RANK))
eng.runner.capture_graphs()
be = EngineLLM(eng, max_new_tokens=16)
sch = eng.scheduler
sch.gather_max_s = 0.0


def decode_batch(B):
    seqs = [Sequence(prompt_ids=be.prompt_ids(f"list pods in namespace team-{i}"),
                     params=SamplingParams(max_new_tokens=64, ignore_eos=True), forced_prefix=list(be._forced))
            for i in range(B)]
    for s in seqs:
        sch.add(s)
    for _ in range(20):
        batch = sch.schedule()
        if batch.is_decode and len(batch.seqs) == B:
            return seqs, batch
        eng._apply(batch, eng.runner.execute(batch))
        sch.on_step_done(batch)
    raise RuntimeError("no full decode batch after 20 steps")


def step_ms(batch, n=int(os.environ.get("MS_N", "30"))):
    for _ in range(5):
        eng.runner.execute(batch)
    if DEV == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        eng.runner.execute(batch)    # ends in a stream synchronise
    return (time.perf_counter() - t0) / n * 1e3


stage = eng.runner._stage_adapter


def stage_none(batch, rows, num_query=None):
    """The plain route without adapter rows: every row -1."""
    eng.runner.stats["lora_steps"] += 1
    return torch.full((rows,), -1, dtype=torch.int32, device=eng.runner.device)


for B in BS:
    seqs, batch = decode_batch(B)
    r = {}
    for rnd in range(2):
        for name, slots, hook in (("graph_base_ms", lambda i: None, stage),
                                  ("plain_route_no_adapter_rows_ms", lambda i: None, stage_none),
                                  ("adapter_half_rows_ms", lambda i: 0 if i % 2 == 0 else None, stage),
                                  ("adapter_all_rows_ms", lambda i: 0, stage)):
            for i, s in enumerate(seqs):
                s.params = SamplingParams(max_new_tokens=64, ignore_eos=True, adapter=slots(i))
            eng.runner._stage_adapter = hook
            before = dict(eng.runner.stats)
            r.setdefault(name, []).append(round(step_ms(batch), 3))
            d = {k: eng.runner.stats[k] - before[k] for k in ("graph_replays", "lora_steps")}
            if name == "graph_base_ms":   # the checked condition: the base path replays graphs, no adapter step
                assert DEV != "cuda" or (d["lora_steps"] == 0 and d["graph_replays"] > 0), d
                r["graph_base_counts"] = d
            else:
                assert d["lora_steps"] > 0 and d["graph_replays"] == 0, (name, d)
    eng.runner._stage_adapter = stage
    res[f"decode_B{B}"] = r
    print(B, r, flush=True)
    for s in seqs:   # retire the batch
        s.params = SamplingParams(max_new_tokens=64, ignore_eos=True)
        eng._finish(s, SeqStatus.FINISHED, "length")
    sch.drop_finished()
    save()
print("done")
