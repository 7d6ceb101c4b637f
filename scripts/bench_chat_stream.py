"""Chat serving latency: streamed and plain chat requests, in-process and through one replica process.

    python scripts/bench_chat_stream.py [--model llama3-8b] [--tokens 32] [--rounds 3]

For C = 1, 8 and 64 closed-loop clients, each sending `--rounds` chat requests of `--tokens` tokens one after the
other, against (a) one engine replica process behind DPRouterLLM, the deployed topology, and (b) EngineLLM in
this process.  The backends' own methods are driven (`generate_chat`, `stream_chat`): the engine, the settle hook,
the IPC and the detokenising are in the figures, HTTP and JSON encoding are not.  Prints, per mode and C, the time
to the first content event, the p50 gap between content events and the p50 total, in ms, and the mean completion
length (random-init weights may reach EOS early).  The replica runs first and is stopped before this process builds
its own engine, so the two never share the device.
"""
import argparse
import asyncio
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLIENTS = (1, 8, 64)
BUCKETS = "1,2,4,8,16,32,48,64"


def _messages(i: int):
    return [{"role": "user", "content": f"describe what pod number {i} in namespace team-{i % 7} is doing"}]


async def _client(backend, i: int, rounds: int, tokens: int, stream: bool, out: list) -> None:
    for r in range(rounds):
        t0 = time.perf_counter()
        if not stream:
            _, _, _, n_out = await backend.generate_chat(_messages(i * 1000 + r), max_tokens=tokens)
            out.append((None, [], time.perf_counter() - t0, n_out))
            continue
        first, gaps, last, n_out = None, [], None, 0
        async for ev in backend.stream_chat(_messages(i * 1000 + r), max_tokens=tokens):
            now = time.perf_counter()
            if "text" in ev:
                if first is None:
                    first = now - t0
                else:
                    gaps.append(now - last)
                last = now
            elif "completion_tokens" in ev:
                n_out = ev["completion_tokens"]
        out.append((first, gaps, time.perf_counter() - t0, n_out))


async def _measure(backend, name: str, args) -> list:
    await backend.start()
    rows = []
    await _client(backend, 0, 2, args.tokens, True, [])   # warm-up: the first request of each path
    await _client(backend, 0, 2, args.tokens, False, [])
    for c in CLIENTS:
        for stream in (False, True):
            out: list = []
            await asyncio.gather(*[_client(backend, i, args.rounds, args.tokens, stream, out) for i in range(c)])
            ms = lambda xs: round(1000 * statistics.median(xs), 2) if xs else None   # noqa: E731
            row = {"backend": name, "clients": c, "stream": stream, "requests": len(out),
                   "first_content_ms_p50": ms([o[0] for o in out if o[0] is not None]),
                   "inter_chunk_ms_p50": ms([g for o in out for g in o[1]]),
                   "total_ms_p50": ms([o[2] for o in out]),
                   "completion_tokens_mean": round(statistics.mean(o[3] for o in out), 1)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", default="cuda:0", help="the replica's device (cpu: a dry run of the script)")
    ap.add_argument("--skip-replica", action="store_true")
    ap.add_argument("--skip-in-process", action="store_true")
    args = ap.parse_args()
    os.environ.setdefault("KV_CACHE_TOKENS", "65536")
    os.environ.setdefault("MAX_MODEL_LEN", "512")

    from ai_agent_kubectl_amd.config import Settings
    s = Settings(LLM_BACKEND="engine", MODEL=args.model, MAX_BATCH=max(CLIENTS), MAX_NEW_TOKENS=args.tokens,
                 HIPGRAPH_BUCKETS=BUCKETS)

    if not args.skip_replica:
        # spawned before this process touches the GPU
        from ai_agent_kubectl_amd.parallel.dp import DPRouterLLM
        t0 = time.perf_counter()
        router = DPRouterLLM(s, 1, devices=[args.device])
        if not router.wait_ready() or not router.replicas[0].up:
            sys.exit("the replica did not start")
        print(json.dumps({"backend": "replica", "start_s": round(time.perf_counter() - t0, 1)}), flush=True)

        async def through_replica():
            try:
                return await _measure(router, "replica", args)
            finally:
                await router.close()

        asyncio.run(through_replica())

    if not args.skip_in_process:
        from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
        from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
        t0 = time.perf_counter()
        eng = build_engine(EngineOptions.from_settings(s))
        eng.runner.capture_graphs()
        backend = EngineLLM(eng, max_new_tokens=args.tokens)
        print(json.dumps({"backend": "in-process", "start_s": round(time.perf_counter() - t0, 1)}), flush=True)

        async def in_process():
            try:
                return await _measure(backend, "in-process", args)
            finally:
                await backend.close()

        asyncio.run(in_process())


if __name__ == "__main__":
    main()
