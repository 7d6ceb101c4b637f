"""Cost of the logprobs path: ops.token_logprobs vs ops.masked_argmax and temperature-only ops.sample, and an
eager logprobs decode step vs the eager sampled step and the graph replay."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, SeqStatus, Sequence  # noqa: E402
from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM  # noqa: E402

DEV = os.environ.get("MS_DEVICE", "cuda")
MODEL = os.environ.get("MS_MODEL", "llama3-8b")
BS = tuple(int(b) for b in os.environ.get("MS_BS", "1,256").split(",") if b)
OUT = os.environ.get("MS_OUT", os.path.join(ROOT, "profiles", "logprobs"))
os.makedirs(OUT, exist_ok=True)
res = {}


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


def save():
    with open(os.path.join(OUT, "bench_logprobs.json"), "w") as f:
        json.dump(res, f, indent=1)


V = 128256
for R in ((1, 64, 256) if DEV == "cuda" else ()):
    torch.manual_seed(R)
    logits = torch.randn(R, V, device=DEV, dtype=torch.bfloat16)
    ties = torch.ones(R, V, device=DEV, dtype=torch.bfloat16)   # one key holds the row: the worst case of the tie scan
    seed = torch.arange(R, dtype=torch.int64, device=DEV)
    pos = torch.arange(R, dtype=torch.int32, device=DEV) % 16
    one, zero = torch.ones(R, device=DEV), torch.zeros(R, dtype=torch.int32, device=DEV)
    t = torch.full((R,), 0.8, device=DEV)
    tok, _ = ops.masked_argmax(logits, None, None)
    r = {}
    for rnd in range(2):   # alternate, two rounds
        r.setdefault("masked_argmax_us", []).append(dev_time(lambda: ops.masked_argmax(logits, None, None)))
        r.setdefault("sample_temp_us", []).append(dev_time(lambda: ops.sample(logits, None, None, t, zero, one, seed, pos)))
        for n in (0, 5, 20):
            r.setdefault(f"logprobs_top{n}_us", []).append(dev_time(lambda: ops.token_logprobs(logits, None, None, tok, n)))
        r.setdefault("logprobs_top20_all_ties_us", []).append(dev_time(lambda: ops.token_logprobs(ties, None, None, tok, 20)))
    res[f"ops_rows{R}"] = {k: [round(x, 1) for x in v] for k, v in r.items()}
    print(R, res[f"ops_rows{R}"], flush=True)
save()

if not BS:
    print("done")
    sys.exit(0)

# ---- engine: eager logprobs decode step vs eager sampled step and graph replay (Llama-3-8B, B = 1 and 256) ----
eng = build_engine(EngineOptions(model=MODEL, device=DEV, max_batch=256, graph_buckets=(1, 2, 256),
                                 kv_cache_tokens=49152, max_model_len=1024, max_batched_tokens=16384, use_graphs=True))
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
        print("step", len(batch.seqs), batch.is_decode, flush=True)
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


for B in BS:
    seqs, batch = decode_batch(B)
    r = {}
    for rnd in range(2):
        for name, kw in (("graph_replay_ms", None), ("eager_temp_ms", dict(temperature=0.8)),
                         ("eager_logprobs0_ms", dict(logprobs=0)), ("eager_logprobs5_ms", dict(logprobs=5)),
                         ("eager_logprobs20_ms", dict(logprobs=20)),
                         ("eager_temp_logprobs20_ms", dict(temperature=0.8, logprobs=20))):
            for s in seqs:
                s.params = SamplingParams(max_new_tokens=64, ignore_eos=True, **(kw or {}))
            before = dict(eng.runner.stats)
            r.setdefault(name, []).append(round(step_ms(batch), 3))
            d = {k: eng.runner.stats[k] - before[k] for k in ("graph_replays", "sampled_steps", "logprob_steps")}
            want_lp = kw is not None and "logprobs" in kw
            assert DEV != "cuda" or ((d["graph_replays"] > 0) == (kw is None) and (d["logprob_steps"] > 0) == want_lp), d
    res[f"decode_B{B}"] = r
    print(B, r, flush=True)
    for s in seqs:   # retire the batch
        s.params = SamplingParams(max_new_tokens=64, ignore_eos=True)
        eng._finish(s, SeqStatus.FINISHED, "length")
    sch.drop_finished()
    save()
print("done")
