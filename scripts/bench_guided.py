"""Timings of guided decoding on one GPU: `ops.guide_mask` alone (device events, warm-up, many launches) at
V = 128256 for 1 / 64 / 256 guided rows with a 16-state and a 2048-state guide, next to `ops.sample` on the same
rows; and the synchronous eager decode step of a batch with one sampled request, without and with a guide on that
request (llama3-8b-2l: the difference is the sampler-side cost, which does not depend on the layer count).
`--baseline-steps` measures only the sampled step and also runs on the parent commit's tree.
Prints one JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ai_agent_kubectl_amd import ops  # noqa: E402
try:
    from ai_agent_kubectl_amd.engine import guided  # noqa: E402
except ImportError:   # a tree from before guided decoding: only `--baseline-steps` (the sampled step) runs there
    guided = None
from ai_agent_kubectl_amd.engine.safe_decode import build_masks  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402
from ai_agent_kubectl_amd.engine.tokenizer import SyntheticTokenizer  # noqa: E402

DEV = "cuda"


def timed(fn, warm=20, iters=200):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def kernels():
    tok = SyntheticTokenizer()
    V = tok.vocab_size
    tb = ops.token_table(tok.id_to_bytes, tok.eos_ids, DEV)
    base_bits = torch.from_numpy(build_masks(tok).view(np.int32)).to(DEV)
    table = guided.GuideTable(8192, DEV)
    small = guided.compile_regex(r"kube(ctl)? (get|top) [a-z]+")
    big = guided.compile_regex(r"[a-z -]{1,2046}")
    assert big.nstates == 2047, big.nstates
    for name, g in (("%d-state" % small.nstates, small), ("%d-state" % big.nstates, big)):
        p = table.acquire(g)
        table.flush()
        for rows in (1, 64, 256):
            i32 = lambda v: torch.full((rows,), v, dtype=torch.int32, device=DEV)   # noqa: E731
            # rows spread over the guide's states; the pending token of every row is one that keeps its state
            # alive (a random one would kill a small guide's state and the kernel would skip the walk)
            state = (torch.arange(rows, dtype=torch.int32, device=DEV) * 7) % min(p.nstates, 1024)
            live = [next(t for t in range(128000) if tok.id_to_bytes[t] and g.walk(s, tok.id_to_bytes[t]) >= 0)
                    for s in range(min(p.nstates, 1024))]
            tokens = torch.tensor([live[s] for s in state.tolist()], dtype=torch.int32, device=DEV)
            pend = torch.arange(rows, dtype=torch.int32, device=DEV)
            for with_base in (False, True):
                args = (tb, table.trans, table.accept, i32(p.base), i32(p.nstates), state, pend, tokens,
                        base_bits if with_base else None, i32(1) if with_base else None)
                us = timed(lambda: ops.guide_mask(*args))
                bits, idx, after = ops.guide_mask(*args)
                allowed = int(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in bits[idx[0]].tolist()))
                print(json.dumps(dict(op="guide_mask", guide=name, rows=rows, safe_mask=with_base, us=round(us, 2),
                                      allowed_row0=allowed, live_rows=int((after >= 0).sum()))), flush=True)
            logits = torch.randn(rows, V, device=DEV).to(torch.bfloat16)
            f = lambda v: torch.full((rows,), v, dtype=torch.float32, device=DEV)   # noqa: E731
            sargs = (logits, bits, idx, f(0.8), i32(0), f(1.0), torch.arange(rows, dtype=torch.int64, device=DEV), i32(3))
            print(json.dumps(dict(op="sample (the sampler the mask feeds)", guide=name, rows=rows,
                                  us=round(timed(lambda: ops.sample(*sargs)), 2))), flush=True)


def steps(with_guide=True):
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=256, graph_buckets=(1, 64, 256),
                                     kv_cache_tokens=65536, max_model_len=256))
    eng.runner.capture_graphs()
    be = EngineLLM(eng, max_new_tokens=8)
    g = guided.compile_regex(r"kubectl (get|describe) (pods|nodes|svc) -n [a-z0-9-]+") if with_guide else None
    sch = eng.scheduler
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    for B in (1, 64, 256):
        for label, guide in (("sampled", None), ("sampled + guided", g))[:2 if with_guide else 1]:
            eng.bm.reset_prefix_cache()
            plain = SamplingParams(max_new_tokens=40, ignore_eos=True)
            kw = dict(guide=guide) if guide is not None else {}
            first = SamplingParams(max_new_tokens=40, ignore_eos=True, safe_decode=False, temperature=0.8, seed=1, **kw)
            seqs = [Sequence(prompt_ids=be.prompt_ids("list pods"), params=first)]
            seqs += [Sequence(prompt_ids=be.prompt_ids("get nodes %d" % i), params=plain, forced_prefix=list(be._forced))
                     for i in range(B - 1)]
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
    if "--baseline-steps" in sys.argv:   # the sampled step alone: also runs on a tree without guided decoding
        steps(with_guide=False)
    else:
        kernels()
        if "--kernels-only" not in sys.argv:
            steps()
