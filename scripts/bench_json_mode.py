"""Timings of JSON mode on one GPU.  `ops.guide_mask_stack` (csrc/guide_stack.hip) at V = 128256 for 1 / 64 / 256
rows spread over the states of the json_object guide, at stack depths 1..40, against `ops.guide_mask`
(csrc/guide_mask.hip, the yardstick) on the same token table with a regex guide of a similar state count, and the
stack kernel on that regex guide's rows as kind 0 (what a DFA row costs when a JSON row shares its step).  Then the
synchronous eager decode step of a batch whose first request samples, without a guide and with the json_object
guide (llama3-8b-2l: the difference is sampler-side and does not depend on the layer count), at B = 1 and 64.
Device events around many launches after a warm-up; three repeats, the median and the spread are printed.
Prints one JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine import guided  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402
from ai_agent_kubectl_amd.engine.tokenizer import SyntheticTokenizer  # noqa: E402

DEV = "cuda"


def timed(fn, warm=20, iters=200, repeats=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)   # us
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def json_rows(g, rows):
    """Rows spread over the guide: prefixes of a nested document, cut at `rows` different places."""
    doc = json.dumps({"name": "web-1", "labels": {"app": "web", "tier": ["a", "b", {"x": [1, 2.5e3, [[[[["deep"]]]]]]}]},
                      "ready": True, "ports": [[[[80, 443]]]], "note": "é\\n", "n": None}).encode()
    doc = doc[:-1] + b',"more":' + b"[" * 36
    state = np.zeros(rows, dtype=np.int32)
    depth = np.zeros(rows, dtype=np.int32)
    words = np.zeros((rows, 8), dtype=np.uint32)
    for r in range(rows):
        s, stack = g.walk(0, doc[:1 + (r * 37) % (len(doc) - 1)], (), per_token=False)
        assert s >= 0
        state[r], depth[r], words[r] = s, len(stack), guided.pack_stack(stack)
    return state, depth, words


def kernels():
    tok = SyntheticTokenizer()
    tb = ops.token_table(tok.id_to_bytes, tok.eos_ids, DEV)
    table = guided.GuideTable(8192, DEV)
    jg = guided.compile_json_object()
    rx = guided.compile_regex(r"[a-z]{1,20} (get|top|describe) [a-z0-9-]{1,60}")
    pj, pr = table.acquire(jg), table.acquire(rx)
    table.flush()
    print(json.dumps(dict(guides={"json_object": jg.nstates, "regex": rx.nstates})), flush=True)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    for rows in (1, 64, 256):
        i32 = lambda v: torch.full((rows,), v, dtype=torch.int32, device=DEV)   # noqa: E731
        state, depth, words = json_rows(jg, rows)
        sargs = (tb, table.trans, table.accept, table.arena_pop, i32(pj.base), i32(pj.nstates), t32(state), i32(1),
                 t32(depth), t32(words.view(np.int32)))
        rstate = (torch.arange(rows, dtype=torch.int32, device=DEV) * 7) % rx.nstates
        dargs = (tb, table.trans, table.accept, i32(pr.base), i32(pr.nstates), rstate)
        kargs = (tb, table.trans, table.accept, table.arena_pop, i32(pr.base), i32(pr.nstates), rstate, i32(0), i32(0),
                 torch.zeros((rows, 8), dtype=torch.int32, device=DEV))
        res = {}
        for name, fn in (("guide_mask_stack json_object", lambda: ops.guide_mask_stack(*sargs)),
                         ("guide_mask regex (yardstick)", lambda: ops.guide_mask(*dargs)),
                         ("guide_mask_stack regex rows as kind 0", lambda: ops.guide_mask_stack(*kargs))):
            med, lo, hi = timed(fn)
            res[name] = med
            print(json.dumps(dict(op=name, rows=rows, us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2))), flush=True)
        a, b = ops.guide_mask_stack(*kargs), ops.guide_mask(*dargs)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        bits = ops.guide_mask_stack(*sargs)[0]
        print(json.dumps(dict(rows=rows, ratio_stack_over_dfa=round(res["guide_mask_stack json_object"] / res["guide_mask regex (yardstick)"], 3),
                              ratio_kind0_over_dfa=round(res["guide_mask_stack regex rows as kind 0"] / res["guide_mask regex (yardstick)"], 3),
                              allowed_per_row=round(float(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in bits.flatten().tolist())) / rows, 1))),
              flush=True)


def steps():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=64, graph_buckets=(1, 64),
                                     kv_cache_tokens=32768, max_model_len=256))
    eng.runner.capture_graphs()
    be = EngineLLM(eng, max_new_tokens=8)
    g = guided.compile_json_object()
    sch = eng.scheduler
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    for B in (1, 64):
        for label, guide, n_guided in (("sampled", None, 0), ("sampled + json_object", g, 1), ("all rows json_object", g, B)):
            if B == 1 and n_guided == B and label.startswith("all"):
                continue
            eng.bm.reset_prefix_cache()
            plain = SamplingParams(max_new_tokens=40, ignore_eos=True)
            mk = lambda i: SamplingParams(max_new_tokens=40, ignore_eos=True, safe_decode=False, temperature=0.8, seed=1 + i,   # noqa: E731
                                          **(dict(guide=guide) if guide is not None else {}))
            seqs = [Sequence(prompt_ids=be.prompt_ids("list pods %d" % i), params=mk(i)) for i in range(max(1, n_guided))]
            seqs += [Sequence(prompt_ids=be.prompt_ids("get nodes %d" % i), params=plain, forced_prefix=list(be._forced))
                     for i in range(B - len(seqs))]
            for s in seqs:
                sch.add(s)
            ms = []
            while any(not s.finished for s in seqs):
                batch = sch.schedule()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks = eng.runner.execute(batch)
                torch.cuda.synchronize()
                if batch.is_decode and len(batch.seqs) == B:
                    ms.append((time.perf_counter() - t0) * 1e3)
                eng._apply(batch, toks)
                sch.on_step_done(batch)
            ms = sorted(ms[5:])
            print(json.dumps(dict(op="eager decode step", batch=B, request=label, steps=len(ms),
                                  median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4))), flush=True)


if __name__ == "__main__":
    kernels()
    if "--kernels-only" not in sys.argv:
        steps()
