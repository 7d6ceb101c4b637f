"""Cost of the penalty / logit_bias path: ops.logit_adjust (+ ops.logit_restore) per call, the host cost of
building the step's image, and an eager penalised decode step vs the eager sampled step and the graph replay."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine import penalties  # noqa: E402
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, SeqStatus, Sequence  # noqa: E402
from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM  # noqa: E402

DEV = os.environ.get("MS_DEVICE", "cuda")
MODEL = os.environ.get("MS_MODEL", "llama3-8b")
BS = tuple(int(b) for b in os.environ.get("MS_BS", "1,256").split(",") if b)
OUT = os.environ.get("MS_OUT", os.path.join(ROOT, "profiles", "penalties"))
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
    with open(os.path.join(OUT, "bench_penalties.json"), "w") as f:
        json.dump(res, f, indent=1)


# ---- the kernels: rows x entries per row, V = 128256, every row with a pending token ----
V = 128256
for R in ((1, 64, 256) if DEV == "cuda" else ()):
    torch.manual_seed(R)
    logits = torch.randn(R, V, device=DEV, dtype=torch.bfloat16)
    tok, _ = ops.masked_argmax(logits, None, None)
    r = {}
    for n in (16, 512, 8500):
        rs = np.random.RandomState(n)
        ids = np.stack([rs.permutation(V)[:n] for _ in range(R)]).astype(np.int32).reshape(-1)
        t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
        row_start = t(np.arange(R + 1, dtype=np.int32) * n)
        ent_id, ent_cnt = t(ids), t(rs.randint(0, 4, size=R * n).astype(np.int32))
        ent_bias = t((rs.rand(R * n) < 0.03).astype(np.float32) * 5.0)
        pres, freq, rep = (torch.full((R,), v, device=DEV) for v in (0.5, 0.3, 1.2))
        pend = torch.arange(R, dtype=torch.int32, device=DEV)
        args = (row_start, ent_id, ent_cnt, ent_bias, pres, freq, rep, pend, tok)

        def both():
            saved = ops.logit_adjust(logits, *args, save=True)
            ops.logit_restore(logits, row_start, ent_id, pres, freq, rep, pend, tok, saved)

        def both_kernels_only(saved=torch.zeros(R + R * n, dtype=torch.bfloat16, device=DEV)):
            lib = ops.require()
            p = ops._p
            ops.check(lib.ka_logit_adjust(p(logits), p(row_start), p(ent_id), p(ent_cnt), p(ent_bias), p(pres), p(freq),
                                          p(rep), p(pend), p(tok), R, p(saved), R, R * n, V, 0, ops._stream()), "adjust")
            ops.check(lib.ka_logit_restore(p(logits), p(row_start), p(ent_id), p(pres), p(freq), p(rep), p(pend), p(tok),
                                           R, p(saved), R, R * n, V, 0, ops._stream()), "restore")

        for rnd in range(2):   # alternate, two rounds
            r.setdefault(f"adjust_{n}_us", []).append(dev_time(lambda: ops.logit_adjust(logits, *args)))
            r.setdefault(f"adjust_save_restore_{n}_us", []).append(dev_time(both))
            r.setdefault(f"adjust_restore_launches_{n}_us", []).append(dev_time(both_kernels_only))
    for rnd in range(2):
        r.setdefault("masked_argmax_us", []).append(dev_time(lambda: ops.masked_argmax(logits, None, None)))
    res[f"ops_rows{R}"] = {k: [round(x, 1) for x in v] for k, v in r.items()}
    print(R, res[f"ops_rows{R}"], flush=True)
save()

# ---- the host: the image of 256 rows (engine/penalties.py pack_edits), first build and a later step ----
rs = np.random.RandomState(0)
host = {}
for name, n_prompt, kw in (("outputs_only_16", 64, dict(frequency_penalty=0.5)),
                           ("prompt_512", 512, dict(repetition_penalty=1.2)),
                           ("prompt_8192_bias_300", 8192, dict(repetition_penalty=1.2, frequency_penalty=0.5,
                                                               logit_bias={100000 + i: 1.0 for i in range(300)}))):
    seqs = []
    for i in range(256):
        s = Sequence(prompt_ids=rs.permutation(100000)[:n_prompt].tolist(),
                     params=SamplingParams(max_new_tokens=64, ignore_eos=True, **kw))
        s.output_ids = rs.randint(0, 100000, size=16).tolist()
        seqs.append(s)
    t0 = time.perf_counter()
    img, E = penalties.pack_edits(seqs, 256, list(range(256)))
    first = (time.perf_counter() - t0) * 1e3
    later = []
    for step in range(5):
        for s in seqs:
            s.output_ids.append(int(rs.randint(0, 100000)))
        t0 = time.perf_counter()
        img, E = penalties.pack_edits(seqs, 256, list(range(256)))
        later.append((time.perf_counter() - t0) * 1e3)
    host[name] = dict(entries_per_row=E // 256, image_kib=round(img.nbytes / 1024, 1), first_build_ms=round(first, 2),
                      later_step_ms=[round(x, 2) for x in later])
    print("host", name, host[name], flush=True)
res["host_pack_256_rows"] = host
save()

if not BS:
    print("done")
    sys.exit(0)

# ---- engine: eager penalised decode step vs eager sampled step and graph replay (Llama-3-8B, B = 1 and 256) ----
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


BIAS300 = {1000 + i: 1.0 for i in range(300)}
for B in BS:
    seqs, batch = decode_batch(B)
    r = {}
    for rnd in range(2):
        for name, kw in (("graph_replay_ms", None), ("eager_temp_ms", dict(temperature=0.8)),
                         ("eager_frequency_ms", dict(frequency_penalty=0.5)),
                         ("eager_all_four_ms", dict(frequency_penalty=0.5, presence_penalty=0.5, repetition_penalty=1.2,
                                                    logit_bias=BIAS300)),
                         ("eager_temp_all_four_ms", dict(temperature=0.8, frequency_penalty=0.5, presence_penalty=0.5,
                                                         repetition_penalty=1.2, logit_bias=BIAS300)),
                         ("eager_all_four_logprobs5_ms", dict(frequency_penalty=0.5, presence_penalty=0.5,
                                                              repetition_penalty=1.2, logit_bias=BIAS300, logprobs=5))):
            for s in seqs:
                s.params = SamplingParams(max_new_tokens=64, ignore_eos=True, **(kw or {}))
                s.penalty_state = None
            before = dict(eng.runner.stats)
            r.setdefault(name, []).append(round(step_ms(batch), 3))
            d = {k: eng.runner.stats[k] - before[k] for k in ("graph_replays", "sampled_steps", "penalty_steps")}
            want_pen = kw is not None and "frequency_penalty" in kw
            assert DEV != "cuda" or ((d["graph_replays"] > 0) == (kw is None) and (d["penalty_steps"] > 0) == want_pen), d
    r["entries_per_row_all_four"] = seqs[0].penalty_state.n if seqs[0].penalty_state is not None else 0
    res[f"decode_B{B}"] = r
    print(B, r, flush=True)
    for s in seqs:   # retire the batch
        s.params = SamplingParams(max_new_tokens=64, ignore_eos=True)
        eng._finish(s, SeqStatus.FINISHED, "length")
    sch.drop_finished()
    save()
print("done")
