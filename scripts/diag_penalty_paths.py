"""Where does a seeded request leave its alone-run on the GPU, without and with penalties?

Two records under profiles/penalties/ (tests/test_penalties_gpu.py refers to them):
* diag_threaded_mixed_plain_vs_penalised.log: the same sampled request (T = 0.9, top_k 50, seed 7) alone and in the
  threaded engine beside three other requests, first without and then with the four penalty fields; for the
  penalised run every adjust launch's counts (entries plus the pending token) against the tokens returned.
* diag_preemption_12_seeds.log: seeds 1-12, alone against a two-row synchronous batch with and without a forced
  recompute preemption after four tokens, for the plain request and penalised variants.
"""
import os
import sys
import threading
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402
from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM  # noqa: E402

OUT = os.environ.get("MS_OUT", os.path.join(ROOT, "profiles", "penalties"))
os.makedirs(OUT, exist_ok=True)
Q, N = "list pods in prod", 8
eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                 kv_cache_tokens=4096, max_model_len=256))
eng.runner.capture_graphs()
be = EngineLLM(eng, max_new_tokens=8)
GREEDY = dict(max_new_tokens=N, ignore_eos=True)


def alone(kw):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(Q)], SamplingParams(**kw), forced_prefix=be._forced)[0]


def new_seq(query, kw):
    return Sequence(prompt_ids=be.prompt_ids(query), params=SamplingParams(**kw), forced_prefix=list(be._forced))


def run_sync(seqs, preempt_at=-1):
    eng.bm.reset_prefix_cache()
    sch = eng.scheduler
    saved = (sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps)
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    try:
        step = 0
        for s in seqs:
            sch.add(s)
        while any(not s.finished for s in seqs):
            if step == preempt_at:
                sch._preempt(seqs[0])
            batch = sch.schedule()
            eng._apply(batch, eng.runner.execute(batch))
            sch.on_step_done(batch)
            step += 1
    finally:
        sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = saved
    return seqs


def threaded(kw):
    others = [("get svc -A", dict(max_new_tokens=3, ignore_eos=True)),
              ("top nodes", dict(max_new_tokens=6, ignore_eos=True, frequency_penalty=2.0, logprobs=2)),
              ("describe pod web-1", dict(max_new_tokens=5, ignore_eos=True, temperature=0.7, seed=3))]
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == 4:
            ev.set()
    eng.start()
    try:
        got = [eng.submit(be.prompt_ids(q), SamplingParams(**p), cb, forced_prefix=be._forced)
               for q, p in [others[0], (Q, kw)] + others[1:]]
        assert ev.wait(60)
    finally:
        eng.shutdown()
    return got[1]


# ---- the threaded mixed batch ----
base = dict(max_new_tokens=N, ignore_eos=True, temperature=0.9, top_k=50, seed=7)
plain = alone(base)
pen = dict(base, presence_penalty=0.5, frequency_penalty=1.2, repetition_penalty=1.3,
           logit_bias={plain.generated[2]: -100.0, plain.generated[0]: -0.5, 2000: 4.0})
records, orig = [], ops.logit_adjust


def hook(logits, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src=None, tokens=None, **k):
    records.append([t.clone() for t in (row_start, ent_id, ent_cnt, repetition, pend_src, tokens)])
    return orig(logits, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src, tokens, **k)


with open(os.path.join(OUT, "diag_threaded_mixed_plain_vs_penalised.log"), "w") as f:
    for name, kw in (("plain", base), ("penalised", pen)):
        a = alone(kw)
        records.clear()
        ops.logit_adjust = hook
        try:
            s = threaded(kw)
        finally:
            ops.logit_adjust = orig
        print(name, "alone   ", a.output_ids, file=f)
        print(name, "threaded", s.output_ids, "SAME" if s.output_ids == a.output_ids else "DIFFERENT", file=f)
        if name == "plain":
            continue
        bad = launches = 0
        for rs, ids, cnt, rep, pend, tok in ([t.tolist() for t in r] for r in records):
            for j in range(len(rs) - 1):
                if abs(rep[j] - 1.3) > 1e-6:
                    continue
                c = Counter()
                for t, w in zip(ids[rs[j]:rs[j + 1]], cnt[rs[j]:rs[j + 1]]):
                    if w & 0x7FFFFFFF:
                        c[t] += w & 0x7FFFFFFF
                if pend[j] >= 0:
                    c[tok[pend[j]]] += 1
                n = sum(c.values())
                launches += 1
                bad += c != Counter(s.output_ids[:n])
                print("  launch of", len(rs) - 1, "rows: row", j, "counted", n, "pending slot", pend[j],
                      "OK" if c == Counter(s.output_ids[:n]) else "MISMATCH", file=f)
        print("penalised: adjust launches", launches, "count mismatches", bad, file=f)

# ---- preemption, 12 seeds ----
with open(os.path.join(OUT, "diag_preemption_12_seeds.log"), "w") as f:
    print("per seed 1..12: (first index that differs from the alone-run after a preemption, -1 = none; "
          "same as the alone-run in a two-row batch without a preemption)", file=f)
    for name, extra in (("plain", {}), ("frequency 1.2", dict(frequency_penalty=1.2)),
                        ("repetition 1.3", dict(repetition_penalty=1.3)), ("bias", dict(logit_bias={2000: 4.0})),
                        ("temperature 0, repetition 1.3 (one request: the seed is ignored)",
                         dict(repetition_penalty=1.3, temperature=0.0))):
        out = []
        for seed in range(1, 13):
            p = dict(dict(max_new_tokens=N, ignore_eos=True, temperature=0.9, top_k=50, seed=seed), **extra)
            a = alone(p).output_ids
            b = run_sync([new_seq(Q, p), new_seq("get nodes -o wide", GREEDY)], preempt_at=4)[0].output_ids
            c = run_sync([new_seq(Q, p), new_seq("get nodes -o wide", GREEDY)])[0].output_ids
            out.append((next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), -1), a == c))
        print(name, out, file=f)
print("done")
