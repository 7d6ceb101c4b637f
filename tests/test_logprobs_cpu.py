"""Per-token log-probabilities on the CPU: the reference's definition (ops/reference.py `token_logprobs`), the
engine's records (aligned with the generated tokens through every launch path) and the
/v1/chat/completions fields.  The HIP kernel is in test_logprobs_gpu.py."""
import threading

import numpy as np
import pytest
import torch

from ai_agent_kubectl_amd import ops
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence
from ai_agent_kubectl_amd.ops import reference as ref
from tests import logprob_cases as lc
from tests import sampling_cases as sc

BF = torch.bfloat16


# ---------------- the reference ----------------
@pytest.mark.parametrize("case", [c for c in sc.CASES if c[0] <= 520], ids=lc.case_id)
def test_probabilities_sum_to_one_and_fp32_is_within_tolerance(case):
    inp, want = lc.build(case)
    V, R, off, masked = case
    # exp(logprob) over A sums to 1: ask for every token of the slice as the chosen one
    for r in range(R):
        rep = lambda t: t[r:r + 1].expand(V, *t.shape[1:]).contiguous()   # noqa: E731
        tok = torch.arange(off, off + V, dtype=torch.int32)
        lp, _, _ = ref.token_logprobs(rep(inp["logits"]), inp["bits"], rep(inp["midx"]) if masked else None, tok, 0, off,
                                      dtype=torch.float64)
        assert int(torch.isfinite(lp).sum()) == int(want["count"][r])
        assert abs(float(lp.exp().sum()) - 1.0) < 1e-5
        if r == 2:
            break
    # the fp32 form of the definition (what ops.token_logprobs runs on CPU tensors) against float64
    lp, tid, tlp, mx, cnt, mass = ops.token_logprobs(inp["logits"], inp["bits"], inp["midx"], inp["token"], 20, off,
                                                     return_probe=True)
    assert lp.dtype == torch.float32 and tid.dtype == torch.int32 and mass.dtype == torch.int64
    assert torch.equal(tid, want["top_id"]) and torch.equal(cnt, want["count"]) and torch.equal(mx, want["max"])
    lc.check_close(lp, want["lp"])
    lc.check_close(tlp, want["top_lp"])
    lc.check_mass(mass, want, V)


def test_mask_and_vocab_offset():
    V, off = 64, 64
    logits = lc.make_logits(2, V, 1)
    bits = torch.zeros(1, 4, dtype=torch.int32)
    allowed = [off + 3, off + 9, off + 40]
    for g in allowed:
        bits[0, g // 32] |= 1 << (g % 32)
    bits[0, 0] = -1   # ids below the slice: must not count
    midx = torch.tensor([0, -1], dtype=torch.int32)
    tok = torch.tensor([off + 9, off + 9], dtype=torch.int32)
    lp, tid, tlp, mx, cnt, _ = ref.token_logprobs(logits, bits, midx, tok, 5, off, return_probe=True, dtype=torch.float64)
    assert cnt.tolist() == [3, V]
    assert sorted(tid[0, :3].tolist()) == allowed and tid[0, 3:].tolist() == [-1, -1]
    la = logits[0].double()[[3, 9, 40]]
    assert float(mx[0]) == float(la.max())
    assert torch.allclose(lp[0], torch.log_softmax(la, 0)[1], atol=1e-9)
    assert torch.allclose(lp[1], torch.log_softmax(logits[1].double(), 0)[9], atol=1e-9)
    assert bool((tid[1] >= off).all()) and bool((tid[1] < off + V).all())


def test_ties_go_to_the_lowest_id_and_top_n_is_a_prefix():
    l = torch.tensor([[1.0, 3.0, 2.0, 3.0, 2.0, 2.0, -1.0, 0.5, 3.0, 0.0, -0.0, 0.0, 2.0, 1.0, 1.0, 1.0]], dtype=BF)
    tok = torch.tensor([1], dtype=torch.int32)
    _, t20, l20 = ref.token_logprobs(l, None, None, tok, 20)
    assert t20[0, :16].tolist() == [1, 3, 8, 2, 4, 5, 12, 0, 13, 14, 15, 7, 9, 10, 11, 6]   # -0 ties with +0
    assert t20[0, 16:].tolist() == [-1] * 4 and bool(torch.isinf(l20[0, 16:]).all())
    for n in (0, 1, 2, 3, 4, 5, 7, 16):
        lp, tn, ln = ref.token_logprobs(l, None, None, tok, n)
        assert tn.shape == (1, n) and torch.equal(tn, t20[:, :n]) and torch.equal(ln, l20[:, :n])
        assert float(lp[0]) == float(l20[0, 0])
    # all equal: the n lowest ids
    _, t, lp = ref.token_logprobs(torch.zeros(1, 32, dtype=BF), None, None, tok, 5)
    assert t[0].tolist() == [0, 1, 2, 3, 4] and torch.allclose(lp, torch.full((1, 5), -float(np.log(32.0))))


def test_fewer_allowed_than_top_n_and_out_of_set_tokens():
    inp, want = lc.build((8, 3, 0, True))
    c = int(want["count"][0])
    assert 0 < c < 5
    assert want["top_id"][0, c:].tolist() == [-1] * (20 - c) and bool(torch.isinf(want["top_lp"][0, c:]).all())
    bits = inp["bits"].numpy().view("uint32")
    banned = next(g for g in range(8) if not (int(bits[0, g // 32]) >> (g % 32)) & 1)
    for t in (banned, -1, 8, 10 ** 6):
        tok = torch.tensor([t, 0, 0], dtype=torch.int32)
        lp, _, _ = ref.token_logprobs(inp["logits"], inp["bits"], inp["midx"], tok, 0)
        assert float(lp[0]) == float("-inf")
    assert float(want["lp"][1]) > float("-inf")   # row 1 is unmasked


def test_weights_below_two_to_the_minus_forty_count_as_zero():
    inp, want = lc.dominated()
    lp, tid, tlp, _, _, mass = ops.token_logprobs(inp["logits"], None, None, inp["token"], 20, inp["off"],
                                                  return_probe=True)
    assert mass.tolist() == [1 << 40] * 3 and want["mass"].tolist() == [1 << 40] * 3
    assert float(lp[0]) == 0.0 and bool((tlp[:, 0] == 0.0).all())
    with pytest.raises(ValueError):
        ops.token_logprobs(inp["logits"], None, None, inp["token"], 21)


# ---------------- engine (tiny-llama) ----------------
@pytest.fixture(scope="module")
def tiny():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=8, graph_buckets=(1, 2, 4, 8),
                                     kv_cache_tokens=8192, max_model_len=512))
    return eng, EngineLLM(eng, max_new_tokens=8)


Q = "list pods in prod"
GREEDY5 = dict(max_new_tokens=8, ignore_eos=True, logprobs=5)
SAMPLED3 = dict(max_new_tokens=8, ignore_eos=True, temperature=0.9, top_k=50, top_p=0.95, seed=7, logprobs=3)


def _alone(eng, be, query, params):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params, forced_prefix=be._forced)[0]


def test_records_are_aligned_with_the_generated_tokens(tiny):
    eng, be = tiny
    before = eng.runner.stats["logprob_steps"]
    s = _alone(eng, be, Q, SamplingParams(**GREEDY5))
    assert be._forced and s.n_forced == len(be._forced)     # the jump-forward prefix gets no record
    assert len(s.logprobs) == s.num_generated == len(s.generated) == 8
    assert eng.runner.stats["logprob_steps"] == before + 8 and -1 not in s.output_ids
    for tok, rec in zip(s.generated, s.logprobs):   # greedy: the chosen id is top[0], with its logprob
        assert rec.top_ids[0] == tok and rec.logprob == rec.top_logprobs[0]
        assert len(rec.top_ids) == len(rec.top_logprobs) == 5
        assert rec.top_logprobs == sorted(rec.top_logprobs, reverse=True) and rec.logprob <= 0.0
    # the tokens are what the request generates without logprobs, and such a request records nothing
    g = _alone(eng, be, Q, SamplingParams(max_new_tokens=8, ignore_eos=True))
    assert g.output_ids == s.output_ids and g.logprobs == []
    # logprobs = 0: the chosen token's logprob alone
    z = _alone(eng, be, Q, SamplingParams(max_new_tokens=8, ignore_eos=True, logprobs=0))
    assert [r.logprob for r in z.logprobs] == [r.logprob for r in s.logprobs]
    assert all(r.top_ids == [] and r.top_logprobs == [] for r in z.logprobs)


def test_sampled_request_reports_the_unprocessed_distribution(tiny):
    eng, be = tiny
    s = _alone(eng, be, Q, SamplingParams(**SAMPLED3))
    g = _alone(eng, be, Q, SamplingParams(max_new_tokens=8, ignore_eos=True, logprobs=3))
    assert len(s.logprobs) == 8 and s.output_ids != g.output_ids
    seen = 0
    for tok, rec in zip(s.generated, s.logprobs):
        assert rec.logprob <= 0.0 and np.isfinite(rec.logprob)
        if tok in rec.top_ids:
            seen += 1
            assert rec.logprob == rec.top_logprobs[rec.top_ids.index(tok)]
        else:
            assert rec.logprob <= rec.top_logprobs[-1]
    # the first token follows the same prompt: the same distribution whatever the request samples with
    assert s.logprobs[0].top_ids == g.logprobs[0].top_ids and s.logprobs[0].top_logprobs == g.logprobs[0].top_logprobs


@pytest.mark.parametrize("kw", [GREEDY5, SAMPLED3], ids=["greedy", "sampled"])
def test_records_are_the_same_through_every_launch_path(tiny, kw):
    eng, be = tiny
    want = _alone(eng, be, Q, SamplingParams(**kw))
    # prefill queued, then decode steps chained behind tokens still on the device
    eng.bm.reset_prefix_cache()
    s = sc.new_sequence(be, Q, SamplingParams(**kw))
    assert sc.chain_async(eng, s) == want.output_ids
    assert s.logprobs == want.logprobs and len(s.logprobs) == s.num_generated
    # the threaded engine with lookahead, in the company of greedy requests of other lengths and one that
    # asks for more alternatives: every request's own records
    others = [("get svc -A", SamplingParams(max_new_tokens=3, ignore_eos=True)),
              ("top nodes", SamplingParams(max_new_tokens=6, ignore_eos=True, logprobs=20)),
              ("describe pod web-1", SamplingParams(max_new_tokens=5, ignore_eos=True))]
    alone20 = _alone(eng, be, "top nodes", others[1][1])
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == 4:
            ev.set()

    n0, sch = eng.lookahead_steps, eng.scheduler
    saved = sch.max_batched_tokens, sch.min_chunk
    sch.max_batched_tokens, sch.min_chunk = 40, 4   # chunked prompts: partial rows sample nothing
    eng.start()
    try:
        seqs = [eng.submit(be.prompt_ids(q), p, cb, forced_prefix=be._forced)
                for q, p in [others[0], (Q, SamplingParams(**kw))] + others[1:]]
        assert ev.wait(60)
    finally:
        eng.shutdown()
        sch.max_batched_tokens, sch.min_chunk = saved
    assert eng.lookahead_steps > n0 and eng.healthy
    assert seqs[1].output_ids == want.output_ids and seqs[2].output_ids == alone20.output_ids
    assert all(len(q.logprobs) == (q.num_generated if q.params.logprobs is not None else 0) for q in seqs)
    _same_records(seqs[1].logprobs, want.logprobs)
    _same_records(seqs[2].logprobs, alone20.logprobs)
    assert all(len(r.top_ids) == 20 for r in seqs[2].logprobs)


def _same_records(got, want):
    """Records of the same tokens computed in another batch composition.  The CPU reference's fp32 GEMMs sum in
    another order at another batch shape, so a bf16 logit may land one ulp away (2^-7 below magnitude 2, where
    tiny-llama's logits lie) and log S moves by less than that: the value at every rank of the list agrees to
    2^-6, and so does the id wherever the neighbouring values are further apart than that (near-ties may swap).
    The same composition gives equal records, which the callers assert with ==."""
    tol = 2.0 ** -6
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert abs(a.logprob - b.logprob) <= tol and len(a.top_ids) == len(b.top_ids)
        v = b.top_logprobs
        assert all(abs(x - y) <= tol for x, y in zip(a.top_logprobs, v))
        for j, (x, y) in enumerate(zip(a.top_ids, b.top_ids)):
            clear = (j == 0 or v[j - 1] - v[j] > 2 * tol) and (j + 1 == len(v) or v[j] - v[j + 1] > 2 * tol)
            assert x == y or not clear, (j, x, y)


def test_records_survive_a_preemption(tiny):
    """A sequence preempted after four tokens is prefilled again over prompt + tokens: the four records it
    has stay, the recomputation records nothing twice, and the rest follow."""
    eng, be = tiny
    p = SamplingParams(**SAMPLED3)
    want = _alone(eng, be, Q, p)
    eng.bm.reset_prefix_cache()
    sch = eng.scheduler
    saved = (sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps)
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    seqs = [Sequence(prompt_ids=be.prompt_ids(Q), params=p, forced_prefix=list(be._forced)),
            Sequence(prompt_ids=be.prompt_ids("get nodes -o wide"), params=SamplingParams(max_new_tokens=8, ignore_eos=True),
                     forced_prefix=list(be._forced))]
    try:
        step = 0
        for s in seqs:
            sch.add(s)
        while any(not s.finished for s in seqs):
            if step == 4:
                victim = seqs[0]
                assert victim in sch.running and victim.num_generated == 4 and len(victim.logprobs) == 4
                kept = list(victim.logprobs)
                sch._preempt(victim)
            batch = sch.schedule()
            eng._apply(batch, eng.runner.execute(batch))
            sch.on_step_done(batch)
            assert all(len(s.logprobs) == (s.num_generated if s.params.logprobs is not None else 0) for s in seqs)
            step += 1
    finally:
        sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = saved
    assert seqs[0].output_ids == want.output_ids and seqs[0].logprobs[:4] == kept
    _same_records(seqs[0].logprobs, want.logprobs)
    assert seqs[1].logprobs == []


def test_eos_discards_the_chained_successor_and_its_record(tiny):
    """An EOS is only seen at collect: the decode step already chained behind it is thrown away, record and all."""
    eng, be = tiny
    tok = eng.tokenizer
    ref_run = _alone(eng, be, Q, SamplingParams(**GREEDY5))
    stop_at = ref_run.generated[2]
    orig = tok.is_eos
    tok.is_eos = lambda t: orig(t) or t == stop_at
    try:
        eng.bm.reset_prefix_cache()
        done = threading.Event()
        eng.start()
        try:
            s = eng.submit(be.prompt_ids(Q), SamplingParams(max_new_tokens=8, logprobs=5), lambda q: done.set(),
                           forced_prefix=be._forced)
            assert done.wait(60)
        finally:
            eng.shutdown()
    finally:
        tok.is_eos = orig
    n = ref_run.generated.index(stop_at) + 1
    assert s.finish_reason == "stop" and s.generated == ref_run.generated[:n]
    assert len(s.logprobs) == s.num_generated == n and s.logprobs == ref_run.logprobs[:n]


def test_greedy_only_engine_counts_no_logprob_step_and_tp_is_refused():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=2048, max_model_len=256))
    be = EngineLLM(eng, max_new_tokens=4)
    out = eng.generate_blocking([be.prompt_ids(q) for q in ("list pods", "get nodes")], be.params, forced_prefix=be._forced)
    assert eng.runner.stats["logprob_steps"] == 0 and eng.runner.stats["decode_steps"] > 0
    assert all(s.logprobs == [] for s in out) and eng.runner.last_logprobs is None
    for bad in (-1, 21):
        with pytest.raises(ValueError):
            eng.submit([1, 2, 3], SamplingParams(logprobs=bad), lambda s: None)
    eng.runner.tp_size = 2
    try:
        with pytest.raises(ValueError):
            eng.submit([1, 2, 3], SamplingParams(logprobs=0), lambda s: None)
    finally:
        eng.runner.tp_size = 1


def test_execute_above_the_largest_bucket(tiny):
    """rows > bmax: the synchronous path, with buffers of its own."""
    eng, be = tiny
    want = _alone(eng, be, Q, SamplingParams(**GREEDY5))
    r = eng.runner
    saved, r.bmax = r.bmax, 1
    try:
        eng.bm.reset_prefix_cache()
        out = eng.generate_blocking([be.prompt_ids(q) for q in (Q, "get nodes", "top pods")], SamplingParams(**GREEDY5),
                                    forced_prefix=be._forced)
    finally:
        r.bmax = saved
    assert out[0].output_ids == want.output_ids and all(len(s.logprobs) == 8 for s in out)
    _same_records(out[0].logprobs, want.logprobs)


# ---------------- HTTP ----------------
def _client(be):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.config import Settings
    return TestClient(create_app(Settings(RATE_LIMIT="1000/minute", MODEL="tiny-llama"), backend=be))


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "list pods"}], "max_tokens": 6}


def test_http_logprobs_body(tiny):
    eng, be = tiny
    with _client(be) as c:
        before = eng.runner.stats["logprob_steps"]
        plain = c.post("/v1/chat/completions", json=BODY)
        assert plain.status_code == 200 and eng.runner.stats["logprob_steps"] == before
        assert "logprobs" not in plain.json()["choices"][0]    # not requested: the body it always was
        assert set(plain.json()["choices"][0]) == {"index", "message", "finish_reason"}
        off = c.post("/v1/chat/completions", json=dict(BODY, logprobs=False))
        assert off.status_code == 200 and "logprobs" not in off.json()["choices"][0]
        r = c.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=4))
        assert r.status_code == 200, r.text
        assert eng.runner.stats["logprob_steps"] > before
        ch = r.json()["choices"][0]
        text = ch["message"]["content"]
        assert text == plain.json()["choices"][0]["message"]["content"]   # greedy either way
        content = ch["logprobs"]["content"]
        assert set(ch["logprobs"]) == {"content"} and 0 < len(content) <= 6
        for e in content:
            assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
            assert isinstance(e["token"], str) and e["logprob"] <= 0.0 and bytes(e["bytes"]).decode() == e["token"]
            assert 0 < len(e["top_logprobs"]) <= 4
            for a in e["top_logprobs"]:
                assert set(a) == {"token", "logprob", "bytes"}
            assert e["top_logprobs"][0]["logprob"] == e["logprob"] and e["top_logprobs"][0]["bytes"] == e["bytes"]
        assert bytes(b for e in content for b in e["bytes"]) == text.encode()
        # logprobs alone: entries without alternatives
        r0 = c.post("/v1/chat/completions", json=dict(BODY, logprobs=True))
        assert r0.status_code == 200
        c0 = r0.json()["choices"][0]["logprobs"]["content"]
        assert [e["top_logprobs"] for e in c0] == [[]] * len(content)
        assert [e["logprob"] for e in c0] == [e["logprob"] for e in content]


def test_http_logprobs_validation(tiny):
    eng, be = tiny
    with _client(be) as c:
        for bad in (dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1), dict(top_logprobs=3),
                    dict(logprobs=False, top_logprobs=3)):
            assert c.post("/v1/chat/completions", json=dict(BODY, **bad)).status_code == 422, bad
        assert c.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=20)).status_code == 200
        assert c.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=0)).status_code == 200


def test_http_logprobs_under_tp_are_refused(tiny):
    eng, be = tiny
    eng.runner.tp_size = 2   # stands in for a tensor-parallel engine: submit refuses before anything runs
    try:
        with _client(be) as c:
            r = c.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=2))
            assert r.status_code == 400 and "TP" in r.text
    finally:
        eng.runner.tp_size = 1
