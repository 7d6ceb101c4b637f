"""`stream: true` and `stop` on the GPU engine (llama3-8b-2l, captured graphs, overlapped and lookahead steps): a
streamed reply reassembles to the reply of the same request without `stream` over the real sampling, logprob and
guide kernels; a stop match while the successor step is in flight leaves the engine consistent; and one replica
process on the same GPU serves the same two forms through the router."""
import asyncio

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd.config import Settings  # noqa: E402
from tests.test_chat_serving_cpu import URL, _plain, _reassemble  # noqa: E402

MODEL = "llama3-8b-2l"
BODY = {"model": MODEL, "messages": [{"role": "user", "content": "describe the pod as JSON"}], "max_tokens": 24}
SAMPLED = dict(temperature=0.8, top_p=0.9, top_k=40, seed=7, logprobs=True, top_logprobs=3)
JSON_MODE = dict(response_format={"type": "json_object"}, temperature=0.7, seed=3)
REGEX = dict(guided_regex="[a-z ]{40}", max_tokens=64)
USAGE = dict(stream=True, stream_options={"include_usage": True})


@pytest.fixture(scope="module")
def eng_be():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model=MODEL, device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=4096, max_model_len=256))
    eng.runner.capture_graphs()
    return eng, EngineLLM(eng, max_new_tokens=8)


def _app(be):
    from ai_agent_kubectl_amd.api import create_app
    return create_app(Settings(RATE_LIMIT="100000/minute", MODEL=MODEL), backend=be)


def _idle(eng) -> bool:
    return eng.bm.num_used == 0 and not eng._live and all(p.refs == 0 for p in eng.runner.guide_table.placed.values())


def _regex_with_stop(c, body=BODY):
    """The regex request with a stop string taken from its own solo content T -> (body, T[:T.find(stop)])."""
    solo = _plain(c.post(URL, json=dict(body, **REGEX)))["choices"][0]
    text = solo["message"]["content"]
    assert solo["finish_reason"] == "stop" and len(text) == 40
    stop = text[10:13]
    return dict(body, **REGEX, stop=stop), text[:text.find(stop)]


def test_streamed_replies_reassemble_to_the_plain_ones(eng_be):
    from fastapi.testclient import TestClient
    eng, be = eng_be
    replays = eng.runner.stats["graph_replays"]
    with TestClient(_app(be)) as c:
        cut_body, want = _regex_with_stop(c)
        for body in (dict(BODY), dict(BODY, **SAMPLED), dict(BODY, **JSON_MODE), cut_body):
            plain = _plain(c.post(URL, json=body))
            streamed, deltas = _reassemble(c.post(URL, json=dict(body, **USAGE)))
            assert streamed == plain, body
            assert "".join(deltas) == plain["choices"][0]["message"]["content"]
        assert plain["choices"][0]["message"]["content"] == want and plain["choices"][0]["stop_reason"] == cut_body["stop"]
        assert plain["usage"]["completion_tokens"] < 40
        entries = _plain(c.post(URL, json=dict(BODY, **SAMPLED)))["choices"][0]["logprobs"]["content"]
        assert len(entries) > 0 and all(len(e["top_logprobs"]) == 3 and e["logprob"] <= 0 for e in entries)
    print("graph_replays", eng.runner.stats["graph_replays"] - replays, "chained", eng.chained_steps,
          "lookahead", eng.lookahead_steps)
    assert eng.runner.stats["graph_replays"] > replays   # the plain greedy request decodes on the captured graphs
    assert eng.chained_steps + eng.lookahead_steps > 0   # and steps were queued behind steps still in flight
    assert _idle(eng)


def test_a_stop_match_under_an_in_flight_successor_leaves_the_engine_consistent(eng_be):
    """Four concurrent requests fill the batch (max_batch 4: they are admitted as one prefill step), two of them
    stop early on a string taken from their own text.  Every decode step is queued behind the previous one, so the
    step after a stop match has a row for the sequence that just left; that row is discarded.  Each stream equals
    its own non-streamed answer from the same four requests run concurrently."""
    import httpx
    eng, be = eng_be
    app = _app(be)
    msgs = lambda text: [{"role": "user", "content": text}]   # noqa: E731
    bodies = [dict(BODY, messages=msgs("list the pods"), **REGEX),
              dict(BODY, messages=msgs("describe node a"), **SAMPLED, max_tokens=40),
              dict(BODY, messages=msgs("show services"), **REGEX, temperature=0.9, seed=5),
              dict(BODY, messages=msgs("get namespaces"), max_tokens=40, presence_penalty=0.5, logit_bias={"1000": 4})]

    async def four(bodies, extra):
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as ac:
            return await asyncio.gather(*[ac.post(URL, json=dict(b, **extra)) for b in bodies])

    async def run():
        await be.start()
        sch = eng.scheduler
        saved = (sch.gather_max_s, sch.gather_quiet_s)
        sch.gather_max_s, sch.gather_quiet_s = 0.5, 0.25   # an idle engine admits the four together, as one step
        try:
            first = [_plain(r)["choices"][0] for r in await four(bodies, {})]
            for i in (0, 2):   # the two guided ones stop at characters 10..12 of what they wrote
                text = first[i]["message"]["content"]
                assert first[i]["finish_reason"] == "stop" and len(text) == 40
                bodies[i] = dict(bodies[i], stop=[text[10:13]])
            chained = eng.chained_steps + eng.lookahead_steps
            plain = [_plain(r) for r in await four(bodies, {})]
            assert eng.chained_steps + eng.lookahead_steps > chained
            streamed = [_reassemble(r)[0] for r in await four(bodies, USAGE)]
            return first, plain, streamed
        finally:
            sch.gather_max_s, sch.gather_quiet_s = saved
            await be.close()

    first, plain, streamed = asyncio.run(run())
    assert streamed == plain
    # up to the first stop match the four rows are the batch they were without `stop`, so the request that stops
    # first stops exactly where its own text says; after it left, the others sit beside three rows, not four, and
    # only have to be consistent: no stop string in the content, and the same answer streamed and not
    exact = 0
    for i in (0, 2):
        got, text = plain[i]["choices"][0], first[i]["message"]["content"]
        assert got["finish_reason"] == "stop" and _consistent_stop(got, text[10:13])
        if got["stop_reason"] == text[10:13] and got["message"]["content"] == text[:text.find(text[10:13])]:
            exact += plain[i]["usage"]["completion_tokens"] < 40
    assert exact >= 1
    assert _idle(eng)


def _consistent_stop(choice, stop) -> bool:
    """A choice of a request that sent `stop`: the string is not in the content, and stop_reason names it or is null."""
    return stop not in choice["message"]["content"] and choice["stop_reason"] in (stop, None)


@pytest.fixture(scope="module")
def routed():
    """One replica process on cuda:0 beside the in-process engine: a small KV pool and half the free memory."""
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.parallel.dp import DPRouterLLM
    mp = pytest.MonkeyPatch()
    mp.setenv("KV_CACHE_TOKENS", "4096")
    mp.setenv("MAX_MODEL_LEN", "256")
    s = Settings(LLM_BACKEND="engine", MODEL=MODEL, MAX_BATCH=4, MAX_NEW_TOKENS=8, HIPGRAPH_BUCKETS="1,2,4",
                 GPU_MEM_FRACTION=0.5, RATE_LIMIT="100000/minute")
    try:
        router = DPRouterLLM(s, 1, devices=["cuda:0"], start_timeout=600)
        with TestClient(create_app(s, backend=router)) as c:   # leaving it stops the replica
            yield c, router
    finally:
        mp.undo()


def test_one_replica_process_streams_what_it_answers(routed):
    c, router = routed
    assert router.replicas[0].up
    for body in (dict(BODY, **SAMPLED), _regex_with_stop(c)[0]):
        plain = _plain(c.post(URL, json=body))
        streamed, _ = _reassemble(c.post(URL, json=dict(body, **USAGE)))
        assert streamed == plain, body
    assert plain["choices"][0]["finish_reason"] == "stop" and plain["choices"][0]["stop_reason"] == body["stop"]
    assert router.replicas[0].inflight == 0
