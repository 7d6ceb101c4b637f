"""LoRA adapters per request on the CPU: the reference of ops.lora_add against float64, the PEFT loader and its
refusals, adapter requests in the tiny-llama engine against an engine with merged weights, prefix-cache isolation,
and the HTTP surface (in process and through an engine replica)."""
import json

import pytest
import torch

from ai_agent_kubectl_amd import ops
from ai_agent_kubectl_amd.config import Settings
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence
from ai_agent_kubectl_amd.models import lora as mlora
from ai_agent_kubectl_amd.models.config import get_config
from ai_agent_kubectl_amd.ops import reference as ref
from tests import lora_cases as lc
from tests.virtual_tp import assert_same_or_near_tie

BF = torch.bfloat16
CFG = get_config("tiny-llama")
ALL = tuple(mlora.MODULES)
# name -> (r, alpha, modules, seed, zero_b)
ADAPTERS = {"kube": (8, 16, ALL, 1, False), "alt": (16, 16, ("q_proj", "v_proj", "down_proj"), 2, False),
            "zero": (8, 16, ALL, 3, True)}
PROMPTS = ("list all pods in the prod namespace", "show the logs of the api deployment", "get nodes",
           "describe the ingress of the web service")


@pytest.fixture(scope="module")
def peft(tmp_path_factory):
    """{name: (dir, tensors, scale)} and the LORA_ADAPTERS value."""
    root = tmp_path_factory.mktemp("adapters")
    out = {}
    for name, (r, alpha, mods, seed, zero_b) in ADAPTERS.items():
        t = lc.peft_tensors(CFG, r, mods, seed=seed, zero_b=zero_b)
        out[name] = (lc.write_peft_dir(root / name, t, r, alpha, mods), t, lc.lora_scale(r, alpha))
    return out, ",".join(f"{n}={d}" for n, (d, _, _) in out.items())


def _options(**kw):
    return EngineOptions(model="tiny-llama", device="cpu", max_batch=8, graph_buckets=(1, 2, 4, 8),
                         kv_cache_tokens=4096, max_model_len=256, **kw)


@pytest.fixture(scope="module")
def eng(peft):
    return build_engine(_options(lora_adapters=peft[1]))


def _ids(e, text):
    return e.tokenizer.encode(text)


def _params(adapter=None, n=6):
    return SamplingParams(max_new_tokens=n, ignore_eos=True, safe_decode=False, adapter=adapter)


def _run(e, prompts, adapters, reset=True, n=6):
    """All requests in one batch -> (output ids per request, the sequences)."""
    if reset:
        e.bm.reset_prefix_cache()
    seqs = [Sequence(prompt_ids=list(p), params=_params(a, n)) for p, a in zip(prompts, adapters)]
    for s in seqs:
        e.scheduler.add(s)
    while not all(s.finished for s in seqs):
        batch = e.scheduler.schedule()
        e._apply(batch, e.runner.execute(batch))
        e.scheduler.on_step_done(batch)
    return [list(s.output_ids) for s in seqs], seqs


# ---------------- 1. the reference ----------------
@pytest.mark.parametrize("T,K,widths,R", [(5, 64, (16, 16, 16), 16), (19, 192, (48, 16, 32), 16), (33, 256, (272,), 64)])
def test_reference_against_float64(T, K, widths, R):
    c = lc.real_case(T, K, widths, R=R, n_adapters=3)
    c["scale"][1, 0] = 0.0
    y0 = c["y"].clone()
    got = ref.lora_add(c["y"].clone(), c["x"], c["row_adapter"], c["A"], c["B"], c["scale"], c["seg"])
    assert got.dtype == BF
    # the definition: t rounded to bf16, one rounding of y.  fp32 accumulation moves the unrounded value by far less
    # than a bf16 ulp, so the results agree except where that value sits on a rounding boundary: within one ulp
    want = lc.rounded_truth(c)
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64)).log2().floor().exp2() * 2.0 ** -7
    err = (got.double() - want).abs()
    assert (err <= 0.5 * ulp * (1 + 1e-3)).all(), (err / ulp).max().item()
    assert (got == want.to(BF)).float().mean().item() > 0.99
    # and the issue's bound against the unrounded float64 result, every element
    y_ref, bound = lc.float64_truth(c)
    assert ((got.double() - y_ref).abs() <= bound).all()
    # rows of -1 and scale-0 segments keep their bits
    none = c["row_adapter"] < 0
    assert none.any() and torch.equal(got.view(torch.int16)[none], y0.view(torch.int16)[none])
    a1 = c["row_adapter"] == 1
    if a1.any():
        assert torch.equal(got.view(torch.int16)[a1, :widths[0]], y0.view(torch.int16)[a1, :widths[0]])
    assert ops.lora_add(y0.clone(), c["x"], c["row_adapter"], c["A"], c["B"], c["scale"], c["seg"]).equal(got)


def test_reference_exact_probes_equal_the_rounded_definition():
    for T, K, widths, R, r in lc.EXACT_CASES[::5]:
        c = lc.exact_case(T, K, widths, R, r)
        got = ref.lora_add(c["y"].clone(), c["x"], c["row_adapter"], c["A"], c["B"], c["scale"], c["seg"])
        live = c["row_adapter"] >= 0
        assert torch.equal(got[live].double(), lc.rounded_truth(c)[live].to(BF).double())
        assert (got.view(torch.int16)[~live] == lc.SENTINEL).all()


# ---------------- 2. the loader ----------------
def test_loader_packs_the_fused_segments(peft):
    dirs, spec = peft
    ls = mlora.load_adapters(spec, CFG, 16)
    assert ls.names == list(ADAPTERS) and ls.rank == 16 and len(ls.layers) == CFG.num_layers
    segs = mlora.fused_segments(CFG)
    assert segs["wqkv"] == (0, 256, 384, 512) and segs["w13"] == (0, 512, 1024)
    for ai, name in enumerate(ADAPTERS):
        r, alpha, mods, _, _ = ADAPTERS[name]
        t = dirs[name][1]
        for li in range(CFG.num_layers):
            for m, (fw, s) in mlora.MODULES.items():
                f = ls.layers[li][fw]
                assert f.seg == segs[fw] and f.A.dtype == BF and f.B.dtype == BF and f.scale.dtype == torch.float32
                lo, hi = f.seg[s], f.seg[s + 1]
                if m not in mods:   # a missing module: scale 0, nothing packed
                    assert f.scale[ai, s] == 0 and not f.A[ai, s].any() and not f.B[ai, lo:hi].any()
                    continue
                p = f"base_model.model.model.layers.{li}.{lc.PEFT_PREFIX[m]}.{m}"
                assert f.scale[ai, s].item() == alpha / r
                assert torch.equal(f.A[ai, s, :r].float(), t[p + ".lora_A.weight"])
                assert torch.equal(f.B[ai, lo:hi, :r].float(), t[p + ".lora_B.weight"])
                assert not f.A[ai, s, r:].any() and not f.B[ai, lo:hi, r:].any()   # zero beyond r
    assert mlora.load_adapters("", CFG, 16) is None


def test_loader_scale_rules(tmp_path):
    t = lc.peft_tensors(CFG, 4, ("q_proj",))
    plain = lc.write_peft_dir(tmp_path / "p", t, 4, 32, ("q_proj",))
    rs = lc.write_peft_dir(tmp_path / "r", t, 4, 32, ("q_proj",), use_rslora=True)
    ls = mlora.load_adapters(f"p={plain},r={rs}", CFG, 16)
    sc = ls.layers[0]["wqkv"].scale
    assert sc[0, 0].item() == 8.0 and sc[1, 0].item() == 16.0   # alpha / r, alpha / sqrt(r)
    assert sc[0, 1].item() == 0 and ls.layers[0]["wo"].scale[0, 0].item() == 0


def test_loader_refusals(tmp_path):
    good = lc.peft_tensors(CFG, 8, ("q_proj",))

    def refused(name, reason, tensors=good, r=8, mods=("q_proj",), cfg=CFG, max_rank=16, tp=1, **extra):
        d = lc.write_peft_dir(tmp_path / name, tensors, r, 16, mods, **extra)
        with pytest.raises(mlora.LoraError) as e:
            mlora.load_adapters(f"{name}={d}", cfg, max_rank, tp_size=tp)
        assert name in str(e.value) and reason in str(e.value), str(e.value)

    refused("big", "MAX_LORA_RANK", tensors=lc.peft_tensors(CFG, 32, ("q_proj",)), r=32)
    refused("emb", "embed_tokens", mods=("q_proj", "embed_tokens"))
    refused("head", "lm_head", mods=("lm_head",))
    extra = dict(good)
    extra["base_model.model.model.embed_tokens.lora_A.weight"] = torch.zeros(8, 256)
    refused("embt", "embed_tokens", tensors=extra)
    refused("bias", "bias", bias="all")
    refused("save", "modules_to_save", modules_to_save=["lm_head"])
    refused("dora", "DoRA", use_dora=True)
    bad = dict(good)
    k = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"
    bad[k] = torch.zeros(8, 128)
    refused("shape", "shape", tensors=bad)
    deep = {key.replace("layers.0.", "layers.7."): v for key, v in good.items()}
    refused("deep", "layers", tensors=deep)
    refused("moe", "MoE", cfg=get_config("tiny-mixtral"))
    refused("tp", "TP=2", tp=2)
    with pytest.raises(mlora.LoraError, match="at most 8"):
        mlora.parse_adapters(",".join(f"a{i}=/x" for i in range(9)))
    # ... and at engine build
    d = lc.write_peft_dir(tmp_path / "dora2", good, 8, 16, ("q_proj",), use_dora=True)
    with pytest.raises(ValueError, match="dora2.*DoRA"):
        build_engine(_options(lora_adapters=f"dora2={d}"))
    with pytest.raises(ValueError, match="MoE"):
        build_engine(EngineOptions(model="tiny-mixtral", device="cpu", lora_adapters=f"dora2={d}"))


# ---------------- 3. the engine ----------------
@pytest.fixture(scope="module")
def base_tokens(eng):
    prompts = [_ids(eng, p) for p in PROMPTS]
    return prompts, [_run(eng, [p], [None])[0][0] for p in prompts]


def _merged_engine(tensors, scale):
    e = build_engine(_options())
    m = e.runner.model
    m.W = lc.merged_weights(m.W, CFG, tensors, scale)
    m.layers = [m._layer(i) for i in range(CFG.num_layers)]
    assert m.layers[0]["wqkv"].dtype == torch.float32
    return e


@pytest.mark.parametrize("name", ["kube", "alt"])
def test_adapter_request_matches_the_merged_weights(eng, peft, base_tokens, name):
    prompts, base = base_tokens
    slot = list(ADAPTERS).index(name)
    before = eng.runner.stats["lora_steps"]
    got = [_run(eng, [p], [slot])[0][0] for p in prompts]
    assert eng.runner.stats["lora_steps"] > before
    merged = _merged_engine(peft[0][name][1], peft[0][name][2])
    want = [_run(merged, [p], [None])[0][0] for p in prompts]
    assert_same_or_near_tie(merged, prompts, want, got)
    assert any(g != b for g, b in zip(got, base)), "the adapter does not matter: the comparison shows nothing"


def test_zero_adapter_yields_the_base_tokens(eng, base_tokens):
    prompts, base = base_tokens
    slot = list(ADAPTERS).index("zero")
    assert [_run(eng, [p], [slot])[0][0] for p in prompts] == base


def test_mixed_batch_gives_every_request_its_own_tokens(eng, base_tokens):
    prompts, base = base_tokens
    adapters = [None, 0, 1, 0]
    alone = [_run(eng, [p], [a])[0][0] for p, a in zip(prompts, adapters)]
    assert alone[0] == base[0]
    before = dict(eng.runner.stats)
    got, _ = _run(eng, prompts, adapters)
    assert got == alone
    assert eng.runner.stats["lora_steps"] > before["lora_steps"]
    # a base-only batch afterwards takes no adapter step
    mid = eng.runner.stats["lora_steps"]
    assert _run(eng, prompts[:2], [None, None])[0] == base[:2]
    assert eng.runner.stats["lora_steps"] == mid


def test_submit_refuses_an_adapter_outside_the_loaded_set(eng):
    plain = build_engine(_options())
    for e, bad in ((eng, 3), (eng, -1), (eng, True), (plain, 0)):
        with pytest.raises(ValueError, match="adapter"):
            e.submit([1, 2, 3], _params(bad), lambda s: None)


# ---------------- 4. the prefix cache ----------------
def test_prefix_cache_never_crosses_adapters(eng, peft):
    prompt = _ids(eng, "list every pod of every namespace together with its node, its age and its restart count, "
                       "sorted by the number of restarts")
    assert len(prompt) >= 2 * eng.runner.block_size
    s = Sequence(prompt_ids=list(prompt), params=_params(1))
    tag = 2 << 20
    assert s.cache_ids == [t + tag for t in prompt] and Sequence(prompt_ids=list(prompt), params=_params()).cache_ids == prompt
    eng.bm.reset_prefix_cache()
    out = {}
    order = [("base", None), ("a0 first", 0), ("a0 again", 0), ("a1", 1), ("base again", None)]
    cached = {}
    for label, a in order:
        ids, seqs = _run(eng, [prompt], [a], reset=False)
        out[label], cached[label] = ids[0], seqs[0].num_cached_prompt
    assert cached["base"] == 0 and cached["a0 first"] == 0, cached      # adapter 0 does not hit the base blocks
    assert cached["a0 again"] > 0 and cached["base again"] > 0, cached  # ... each hits its own
    assert cached["a1"] == 0, cached                                    # adapter 1 does not hit adapter 0's
    fresh = build_engine(_options(lora_adapters=peft[1]))
    for label, a in order:
        assert _run(fresh, [prompt], [a])[0][0] == out[label], label
    assert out["a0 first"] == out["a0 again"] and out["base"] == out["base again"]
    assert out["a0 first"] != out["base"]


# ---------------- 5. HTTP ----------------
SETTINGS = dict(LLM_BACKEND="engine", MODEL="tiny-llama", MAX_BATCH=8, MAX_NEW_TOKENS=6, HIPGRAPH_BUCKETS="1,2,4,8",
                RATE_LIMIT="100000/minute")
URL = "/v1/chat/completions"
BODY = {"messages": [{"role": "user", "content": "list pods"}], "max_tokens": 12}


def _chat(c, **kw):
    r = c.post(URL, json=dict(BODY, **kw))
    assert r.status_code == 200, r.text
    return r.json()


def _content(body):
    return body["choices"][0]["message"]["content"], body["choices"][0]["finish_reason"], body["usage"]


def _streamed(c, **kw):
    r = c.post(URL, json=dict(BODY, stream=True, **kw))
    assert r.status_code == 200, r.text
    events = [b[6:] for b in r.text.split("\n\n") if b]
    assert events[-1] == "[DONE]"
    chunks = [json.loads(e) for e in events[:-1]]
    return "".join(ch["choices"][0]["delta"].get("content", "") for ch in chunks if ch["choices"]), chunks[0]["model"]


def test_http_serves_adapters_by_model_name(eng, peft):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    s = Settings(**SETTINGS, LORA_ADAPTERS=peft[1])
    with TestClient(create_app(s, backend=EngineLLM(eng, max_new_tokens=6))) as c:
        models = c.get("/v1/models").json()["data"]
        assert models[0] == {"id": "tiny-llama", "object": "model", "owned_by": "local"}
        assert models[1:] == [{"id": n, "object": "model", "owned_by": "local", "parent": "tiny-llama"} for n in ADAPTERS]
        base = _chat(c, model="tiny-llama")
        before = eng.runner.stats["lora_steps"]
        other = _chat(c, model="no-such-adapter")       # any other name: the base model, the name echoed
        assert other["model"] == "no-such-adapter" and _content(other) == _content(base)
        assert _content(_chat(c)) == _content(base)
        assert eng.runner.stats["lora_steps"] == before
        kube = _chat(c, model="kube")
        assert kube["model"] == "kube" and eng.runner.stats["lora_steps"] > before
        assert _content(kube)[0] != _content(base)[0]
        assert _streamed(c, model="kube") == (_content(kube)[0], "kube")
        assert _streamed(c, model="tiny-llama")[0] == _content(base)[0]
        assert _content(_chat(c, model="zero")) == _content(base)
        # the other chat fields act after the forward: they combine with an adapter
        r = _chat(c, model="kube", temperature=0.7, seed=5, logprobs=True, top_logprobs=2, presence_penalty=0.5,
                  guided_choice=["alpha", "beta"])
        assert r["choices"][0]["message"]["content"] in ("alpha", "beta")


def test_lora_kubectl_routes_the_kubectl_endpoint(eng, peft):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    with pytest.raises(ValueError, match="LORA_KUBECTL"):
        create_app(Settings(**SETTINGS, LORA_ADAPTERS=peft[1], LORA_KUBECTL="nope"), backend=EngineLLM(eng))
    be = EngineLLM(eng, max_new_tokens=6)
    with TestClient(create_app(Settings(**SETTINGS, LORA_ADAPTERS=peft[1]), backend=be)) as c:
        before = eng.runner.stats["lora_steps"]
        assert c.post("/kubectl-command", json={"query": "list all pods"}).status_code == 200
        assert eng.runner.stats["lora_steps"] == before and be.params.adapter is None
    be = EngineLLM(eng, max_new_tokens=6)
    with TestClient(create_app(Settings(**SETTINGS, LORA_ADAPTERS=peft[1], LORA_KUBECTL="alt"), backend=be)) as c:
        assert be.params.adapter == 1
        assert c.post("/kubectl-command", json={"query": "show all services"}).status_code == 200
        assert eng.runner.stats["lora_steps"] > before


@pytest.mark.slow
def test_chat_through_a_replica_reaches_the_adapter(eng, peft):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    from ai_agent_kubectl_amd.parallel.dp import DPRouterLLM
    s = Settings(**SETTINGS, LORA_ADAPTERS=peft[1])
    with TestClient(create_app(s, backend=EngineLLM(eng, max_new_tokens=6))) as local:
        want = {m: _content(_chat(local, model=m)) for m in ("tiny-llama", "kube", "alt")}
        want_stream = _streamed(local, model="kube")
    assert want["kube"][0] != want["tiny-llama"][0]
    router = DPRouterLLM(s, 1, devices=["cpu"], start_timeout=300)
    with TestClient(create_app(s, backend=router)) as c:   # leaving it closes the router, which stops its replica
        for m, w in want.items():
            assert _content(_chat(c, model=m)) == w, m
        assert _streamed(c, model="kube") == want_stream
        assert len(c.get("/v1/models").json()["data"]) == 1 + len(ADAPTERS)
