"""Chat completions as they are deployed, on the tiny CPU model: `stop` and the per-step token hook in the engine,
`stream: true` against the same request without it, and all of it again through engine replica processes behind
the router (parallel/dp.py), whose bodies must equal the in-process backend's."""
import asyncio
import json
import time

import pytest

from ai_agent_kubectl_amd.config import Settings
from ai_agent_kubectl_amd.engine import guided
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence
from ai_agent_kubectl_amd.engine.streaming import stop_cut

URL = "/v1/chat/completions"
BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "list pods"}], "max_tokens": 16}
CHOICE = "héllo ✓ 😀 done"
SETTINGS = dict(LLM_BACKEND="engine", MODEL="tiny-llama", MAX_BATCH=8, MAX_NEW_TOKENS=6, HIPGRAPH_BUCKETS="1,2,4,8",
                RATE_LIMIT="100000/minute")
# the request kinds of the issue; "regex_stop" gets its stop string from the solo content (`_with_stop`)
KINDS = {
    "greedy": dict(),
    "sampled_logprobs": dict(temperature=0.8, top_p=0.9, top_k=40, seed=7, logprobs=True, top_logprobs=3),
    "penalties": dict(presence_penalty=0.6, frequency_penalty=0.4, repetition_penalty=1.3, logit_bias={"1000": 6, "17": -100}),
    "regex_stop": dict(guided_regex="[a-z ]{40}", max_tokens=64),
    "choice": dict(guided_choice=[CHOICE], max_tokens=64),
    "json_object": dict(response_format={"type": "json_object"}, max_tokens=24),
}


@pytest.fixture(scope="module")
def tiny():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions.from_settings(Settings(**SETTINGS)))
    return eng, EngineLLM(eng, max_new_tokens=6)


def _app(be):
    from ai_agent_kubectl_amd.api import create_app
    return create_app(Settings(**SETTINGS), backend=be)


def _client(be):
    from fastapi.testclient import TestClient
    return TestClient(_app(be))


def _events(text: str):
    """The `data:` payloads of a server-sent event stream."""
    blocks = [b for b in text.split("\n\n") if b]
    assert all(b.startswith("data: ") for b in blocks), text[:200]
    return [b[6:] for b in blocks]


def _reassemble(resp, usage=True):
    """A streamed reply -> the body the same request gets without `stream` (id and created aside)."""
    assert resp.status_code == 200 and resp.headers["content-type"].startswith("text/event-stream"), resp.text
    events = _events(resp.text)
    assert events[-1] == "[DONE]"
    chunks = [json.loads(e) for e in events[:-1]]
    assert len({(c["id"], c["created"], c["model"]) for c in chunks}) == 1
    assert all(c["object"] == "chat.completion.chunk" for c in chunks)
    first, body = chunks[0], chunks[1:]
    assert first["choices"] == [{"index": 0, "delta": {"role": "assistant", "content": ""}, "finish_reason": None}]
    tail = None
    if usage:
        tail, body = body[-1], body[:-1]
        assert tail["choices"] == [] and all(c["usage"] is None for c in chunks[:-1])
    else:
        assert all("usage" not in c for c in chunks)
    last, content = body[-1]["choices"][0], [c["choices"][0] for c in body[:-1]]
    assert last["delta"] == {} and last["finish_reason"] in ("stop", "length")
    assert all(c["finish_reason"] is None and set(c["delta"]) == {"content"} for c in content)
    choice = {"index": 0, "message": {"role": "assistant", "content": "".join(c["delta"]["content"] for c in content)},
              "finish_reason": last["finish_reason"]}
    if any("logprobs" in c for c in content):
        choice["logprobs"] = {"content": [e for c in content if "logprobs" in c for e in c["logprobs"]["content"]]}
    if "stop_reason" in last:
        choice["stop_reason"] = last["stop_reason"]
    out = {"object": "chat.completion", "model": first["model"], "choices": [choice]}
    if tail is not None:
        out["usage"] = tail["usage"]
    return out, [c["delta"]["content"] for c in content]


def _plain(resp):
    assert resp.status_code == 200, resp.text
    body = resp.json()
    assert body.pop("id").startswith("chatcmpl-") and body.pop("created") > 0
    return body


def _with_stop(c, kind):
    """The request body of a kind; the regex one first asks for the solo content T and stops at T[10:13]."""
    body = dict(BODY, **KINDS[kind])
    if kind != "regex_stop":
        return body, None
    solo = _plain(c.post(URL, json=body))["choices"][0]
    text = solo["message"]["content"]
    assert solo["finish_reason"] == "stop" and len(text) == 40 and "stop_reason" not in solo
    stop = text[10:13]
    return dict(body, stop=stop), text[:text.find(stop)]


def _check_kind(c, kind):
    body, want = _with_stop(c, kind)
    plain = _plain(c.post(URL, json=body))
    streamed, deltas = _reassemble(c.post(URL, json=dict(body, stream=True, stream_options={"include_usage": True})))
    assert streamed == plain, kind
    choice = plain["choices"][0]
    if kind == "regex_stop":
        assert choice["message"]["content"] == want and choice["finish_reason"] == "stop"
        assert choice["stop_reason"] == body["stop"]
    elif kind == "choice":
        assert choice["message"]["content"] == CHOICE == "".join(deltas) and not any("�" in d for d in deltas)
        assert len(deltas) > 1
    elif kind == "sampled_logprobs":
        entries = choice["logprobs"]["content"]
        assert b"".join(bytes(e["bytes"]) for e in entries).decode("utf-8", "replace") == choice["message"]["content"]
        assert all(len(e["top_logprobs"]) == 3 for e in entries)
    else:
        assert "logprobs" not in choice and "stop_reason" not in choice
    return plain


# ---------------- engine ----------------
def _run(eng, seq):
    eng.bm.reset_prefix_cache()
    eng.scheduler.add(seq)
    while not seq.finished:
        batch = eng.scheduler.schedule()
        eng._apply(batch, eng.runner.execute(batch))
        eng.scheduler.on_step_done(batch)
    return seq


def test_engine_stop_cuts_at_the_reference_and_frees_everything(tiny):
    eng, be = tiny
    tok = eng.tokenizer
    g = guided.compile_regex("[a-z ]{40}")
    eng.runner.guides()
    idle = eng.bm.num_used
    base = dict(max_new_tokens=12, safe_decode=False, logprobs=2, guide=g)
    ids = be.chat_ids(BODY["messages"])
    ref = _run(eng, Sequence(prompt_ids=ids, params=SamplingParams(**base)))
    pieces = [tok.token_bytes(t) for t in ref.output_ids]
    assert len(pieces) > 5 and ref.stop_cut is None and ref.stop_scan is None
    stop = pieces[3] + pieces[4]
    cut, which, used = stop_cut(pieces, [b"\xff\xfe", stop])
    assert which == 1 and 0 < cut and used <= 5

    calls = []
    seq = Sequence(prompt_ids=ids, params=SamplingParams(stop=[b"\xff\xfe", stop], **base))
    seq.guide_ref = eng.runner.guides().acquire(g)
    seq.on_tokens = lambda s, first: calls.append((first, list(s.output_ids), s.finished))
    _run(eng, seq)
    assert seq.finish_reason == "stop" and (seq.stop_cut, seq.stop_match) == (cut, 1)
    assert seq.output_ids == ref.output_ids[:used]                # up to the cut: the output without `stop`
    assert len(seq.logprobs) == seq.num_generated == used
    assert [c[0] for c in calls] == list(range(used))             # once per settled step, before the sequence leaves
    assert all(ids_ == ref.output_ids[:i + 1] and not done for i, (_, ids_, done) in enumerate(calls))
    assert eng.bm.num_used == idle and seq.guide_ref is None
    assert all(p.refs == 0 for p in eng.runner.guide_table.placed.values())
    # a stop match on the token that reaches max_new_tokens is still "stop"
    last = _run(eng, Sequence(prompt_ids=ids, params=SamplingParams(stop=[stop], **dict(base, max_new_tokens=used))))
    assert last.finish_reason == "stop" and last.stop_cut == cut and last.output_ids == seq.output_ids
    with pytest.raises(ValueError):
        eng.submit(ids, SamplingParams(stop=[b""]), None)
    with pytest.raises(ValueError):
        eng.submit(ids, SamplingParams(stop=[b"a"] * 5), None)


def test_one_result_assembly_drops_entries_from_the_cut_on(tiny):
    from ai_agent_kubectl_amd.llm.engine_backend import assemble_chat
    eng, be = tiny
    tok = eng.tokenizer
    ids = tok.encode("get pods now")
    assert len(ids) >= 3
    recs = [(-0.5, [t], [-0.5]) for t in ids]
    pieces = [tok.token_bytes(t) for t in ids]
    whole = b"".join(pieces)
    text, finish, n_in, n_out, content = assemble_chat(tok, ids + [next(iter(tok.eos_ids))], 0, recs + [(-1.0, [0], [-1.0])],
                                                       "stop", None, 7)
    assert (text, finish, n_in, n_out) == (whole.decode(), "stop", 7, len(ids) + 1) and len(content) == len(ids)
    cut = len(pieces[0]) + 1   # inside the second token: its entry stays, the third one's goes
    text, finish, _, n_out, content = assemble_chat(tok, ids, 0, recs, "stop", cut, 7)
    assert text == whole[:cut].decode("utf-8", "replace") and n_out == len(ids) and len(content) == 2
    text, _, _, _, content = assemble_chat(tok, ids, 0, recs, "stop", len(pieces[0]), 7)
    assert text == pieces[0].decode() and len(content) == 1
    # a jump-forward prefix is text without entries
    text, _, _, _, content = assemble_chat(tok, ids, 1, recs[1:], "length", None, 7)
    assert text == whole.decode() and [e["token"] for e in content] == [tok.decode([t]) for t in ids[1:]]


# ---------------- HTTP, in-process ----------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_streamed_reply_reassembles_to_the_plain_reply(tiny, kind):
    eng, be = tiny
    with _client(be) as c:
        _check_kind(c, kind)
    assert eng.bm.num_used == 0


def test_stream_without_usage_and_a_request_without_stop_is_unchanged(tiny):
    eng, be = tiny
    with _client(be) as c:
        plain = _plain(c.post(URL, json=BODY))
        assert set(plain["choices"][0]) == {"index", "message", "finish_reason"}
        streamed, _ = _reassemble(c.post(URL, json=dict(BODY, stream=True)), usage=False)
        assert streamed == {k: v for k, v in plain.items() if k != "usage"}
        # `stop` as a list; EOS / length report null
        text = plain["choices"][0]["message"]["content"]
        r = _plain(c.post(URL, json=dict(BODY, stop=["§§", text[4:6]])))["choices"][0]
        assert r["stop_reason"] == text[4:6] and r["message"]["content"] == text[:text.find(text[4:6])]
        r = _plain(c.post(URL, json=dict(BODY, stop="§§")))["choices"][0]
        assert r["stop_reason"] is None and r["finish_reason"] == "length" and r["message"]["content"] == text


def test_status_codes(tiny):
    eng, be = tiny
    with _client(be) as c:
        for bad in ([], "", ["a"] * 5, ["ok", ""], "x" * 65, "€" * 22, 7, [1], {"a": 1}):
            assert c.post(URL, json=dict(BODY, stop=bad)).status_code == 422, bad
        assert c.post(URL, json=dict(BODY, stop="€" * 21)).status_code == 200   # 63 bytes
        assert c.post(URL, json=dict(BODY, stream_options={"include_usage": True})).status_code == 422
        assert c.post(URL, json=dict(BODY, stream=False, stream_options={})).status_code == 422
        r = c.post(URL, json=dict(BODY, stream=True, guided_regex="(unclosed"))
        assert r.status_code == 400 and r.headers["content-type"].startswith("application/json") and "detail" in r.json()


async def _disconnect_after(app, body, chunks: int):
    """POST `body` to the ASGI app and report the client gone once `chunks` body messages have arrived."""
    got, gone = [], asyncio.Event()
    request = [{"type": "http.request", "body": json.dumps(body).encode(), "more_body": False}]

    async def receive():
        if request:
            return request.pop()
        await gone.wait()
        return {"type": "http.disconnect"}

    async def send(msg):
        if msg["type"] == "http.response.body" and msg.get("body"):
            got.append(msg["body"])
            if len(got) >= chunks:
                gone.set()

    scope = {"type": "http", "asgi": {"version": "3.0"}, "http_version": "1.1", "method": "POST", "path": URL,
             "raw_path": URL.encode(), "query_string": b"", "root_path": "", "scheme": "http",
             "headers": [(b"content-type", b"application/json"), (b"host", b"t")], "client": ("127.0.0.1", 1),
             "server": ("t", 80)}
    await app(scope, receive, send)
    return got


def _idle_within(seconds: float, idle) -> bool:
    deadline = time.monotonic() + seconds
    while time.monotonic() < deadline:
        if idle():
            return True
        time.sleep(0.01)
    return idle()


def test_a_client_that_disconnects_aborts_its_request(tiny):
    eng, be = tiny
    app = _app(be)
    body = dict(BODY, stream=True, max_tokens=200, guided_regex="[a-z ]{1500}")

    async def run():
        await be.start()
        got = await _disconnect_after(app, body, 2)
        return got, eng.steps

    got, steps = asyncio.run(run())
    try:
        assert 2 <= len(got) < 100 and not any(b"[DONE]" in g for g in got)
        assert _idle_within(2.0, lambda: eng.bm.num_used == 0 and not eng._live)
        assert all(p.refs == 0 for p in eng.runner.guide_table.placed.values())
        assert eng.steps - steps < 100   # it did not run to its 200 tokens
    finally:
        asyncio.run(be.close())


# ---------------- through replica processes ----------------
@pytest.fixture(scope="module")
def routed():
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.parallel.dp import DPRouterLLM
    s = Settings(**SETTINGS)
    router = DPRouterLLM(s, 2, devices=["cpu", "cpu"], start_timeout=300)
    from ai_agent_kubectl_amd.api import create_app
    app = create_app(s, backend=router)
    with TestClient(app) as c:   # leaving it closes the router, which stops its replicas
        yield c, router, app


@pytest.mark.slow
@pytest.mark.parametrize("kind", list(KINDS))
def test_router_bodies_equal_the_in_process_backend(tiny, routed, kind):
    eng, be = tiny
    c, router, _ = routed
    with _client(be) as local:
        want = _check_kind(local, kind)
    assert _check_kind(c, kind) == want   # 200 where a router answered 404; plain and streamed, both equal
    assert all(r.inflight == 0 for r in router.replicas)


@pytest.mark.slow
def test_router_mixed_load_errors_and_disconnect(routed):
    import httpx
    c, router, app = routed
    assert c.get("/v1/models").status_code == 200
    r = c.post(URL, json=dict(BODY, guided_regex="(unclosed"))
    assert r.status_code == 400 and "detail" in r.json()
    assert c.post(URL, json=dict(BODY, stream=True, guided_regex="(unclosed")).status_code == 400
    assert c.post(URL, json=dict(BODY, logit_bias={"99999999": 1})).status_code == 400
    solo = {k: _plain(c.post(URL, json=dict(BODY, **KINDS[k]))) for k in ("greedy", "sampled_logprobs", "json_object")}

    async def burst():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as ac:
            jobs = []
            for i in range(12):
                if i % 3 == 2:
                    jobs.append(ac.post("/kubectl-command", json={"query": f"list pods in ns{i}"}))
                else:
                    kind = ("greedy", "sampled_logprobs", "json_object", "greedy")[i % 4]
                    jobs.append(ac.post(URL, json=dict(BODY, **KINDS[kind], stream=i % 2 == 1)))
            return await asyncio.gather(*jobs)

    rs = asyncio.run(burst())
    assert [r.status_code for r in rs] == [200] * 12, [r.text[:80] for r in rs]
    for i, r in enumerate(rs):
        if i % 3 == 2:
            assert "kubectl_command" in r.json()
        elif i % 2 == 1:
            assert _events(r.text)[-1] == "[DONE]"
    # the seeded request's answer does not depend on its company
    assert _plain(rs[4])["choices"] == solo["greedy"]["choices"]
    assert _reassemble(rs[1], usage=False)[0]["choices"] == solo["sampled_logprobs"]["choices"]
    assert all(r.inflight == 0 for r in router.replicas)

    body = dict(BODY, stream=True, max_tokens=200, guided_regex="[a-z ]{1500}")
    got = asyncio.run(_disconnect_after(app, body, 2))
    assert 2 <= len(got) < 100
    assert _idle_within(2.0, lambda: all(r.inflight == 0 for r in router.replicas) and not router._pending)
    assert _plain(c.post(URL, json=BODY)) == solo["greedy"]   # and the replicas serve on
