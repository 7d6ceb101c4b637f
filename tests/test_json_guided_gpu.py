"""csrc/guide_stack.hip (`ops.guide_mask_stack`, JSON mode) against the literal pure-Python reference of
tests/json_guide_cases.py, and JSON-guided requests in the engine beside its captured greedy graphs.

Everything is integer, so every comparison is `torch.equal` on all five outputs (bits with the copied SAFE_DECODE
rows, the zero rows and the bits past V; idx; state, depth and stack after the pending token), per case: V around
the word, the ballot and the workgroup tile and at 128256; 1, 3 and 64 rows; every depth around the stack words,
the per-token push limit from both sides, corrupt rows, every pending and base mode.  Then the launcher's return
codes and the engine.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd.engine import guided  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import json_guide_cases as jc  # noqa: E402

DEV = "cuda"
HIP_INVALID = 1   # hipErrorInvalidValue


@pytest.fixture(autouse=True, scope="module")
def _lib():
    lib = _hip.require()
    assert lib.ka_guide_mask_stack_tile() == jc.TILE   # the geometry the cases straddle is the kernel's
    jc.check_preconditions()


def _want(c):
    return tuple(torch.from_numpy((a.view(np.int32) if a.dtype == np.uint32 else a).copy()).to(DEV) for a in jc.literal(c))


@pytest.mark.parametrize("case", jc.CASES, ids=lambda c: c.id)
def test_mask_matches_the_literal_reference_exactly(case):
    want = _want(case)
    got = jc.run_ops(case, DEV)
    assert got[0].shape == want[0].shape and all(g.dtype == torch.int32 for g in got)
    bad = (got[0] != want[0]).nonzero()
    assert torch.equal(got[0], want[0]), (case.id, len(bad), bad[:5].tolist())
    for name, g, w in zip(("idx", "state_after", "depth_after", "stack_after"), got[1:], want[1:]):
        assert torch.equal(g, w), (name, g.tolist(), w.tolist())
    again = jc.run_ops(case, DEV)
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_launcher_refuses_invalid_arguments():
    lib = _hip.require()
    c = next(x for x in jc.CASES if x.V == jc.TILE - 1 and x.rows == 3 and x.base_bits is not None and x.pend_src is not None)
    tb = jc.token_table(c.V, DEV)

    def dev(a, view=None):
        return torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view))).to(DEV)

    words = (c.V + 31) // 32
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)   # noqa: E731
    t = dict(bits=zeros(2 + c.rows, words), idx=zeros(c.rows), after=zeros(c.rows), dafter=zeros(c.rows),
             safter=zeros(c.rows, 8), rec=tb.rec, ovf=tb.ovf, arena=dev(c.trans, np.int16), accept=dev(c.accept),
             pop=dev(c.pop, np.int16), base=dev(c.row_base), nst=dev(c.row_nstates), st=dev(c.row_state),
             kind=dev(c.row_kind), depth=dev(c.row_depth), stack=dev(c.row_stack, np.int32), pend=dev(c.pend_src),
             tokens=dev(c.tokens), bbits=dev(c.base_bits, np.int32), bidx=dev(c.base_idx))
    good = dict(ovf_bytes=tb.ovf_bytes, vocab=c.V, eos0=c.eos_ids[0], arena_states=c.trans.shape[0],
                n_tokens=len(c.tokens), n_static=2, rows=c.rows)

    def call(**kw):
        a = {k: v.data_ptr() for k, v in t.items()}
        a.update(good)
        a.update(kw)
        return lib.ka_guide_mask_stack(
            a["bits"], a["idx"], a["after"], a["dafter"], a["safter"], a["rec"], a["ovf"], a["ovf_bytes"], a["vocab"],
            a["eos0"], a["arena"], a["accept"], a["pop"], a["arena_states"], a["base"], a["nst"], a["st"], a["kind"],
            a["depth"], a["stack"], a["pend"], a["tokens"], a["n_tokens"], a["bbits"], a["bidx"], a["n_static"],
            a["rows"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    want = _want(c)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(t["bits"][2:], want[0][2:]) and torch.equal(t["dafter"], want[3]) and torch.equal(t["safter"], want[4])
    for name in ("bits", "after", "dafter", "safter"):
        t[name].fill_(0x5A5A5A5A)
    bad = [dict(bits=None), dict(idx=None), dict(after=None), dict(dafter=None), dict(safter=None), dict(rec=None),
           dict(arena=None), dict(accept=None), dict(pop=None), dict(base=None), dict(nst=None), dict(st=None),
           dict(kind=None), dict(depth=None), dict(stack=None), dict(tokens=None), dict(bbits=None), dict(bidx=None),
           dict(ovf=None), dict(n_static=0), dict(bbits=None, bidx=None), dict(rec=t["rec"].data_ptr() + 4),
           dict(pop=t["pop"].data_ptr() + 1), dict(stack=t["stack"].data_ptr() + 2),
           dict(rows=-1), dict(rows=65536), dict(vocab=0), dict(vocab=-5), dict(eos0=-1), dict(eos0=c.V),
           dict(arena_states=0), dict(ovf_bytes=-1), dict(n_tokens=-1), dict(n_static=-1)]
    assert tb.ovf_bytes > 0
    for kw in bad:
        assert call(**kw) == HIP_INVALID, kw
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    for name in ("bits", "after", "dafter", "safter"):
        assert bool((t[name] == 0x5A5A5A5A).all()), name   # none of them launched anything
    assert call(pend=None, tokens=None, n_tokens=0) == 0      # no row has a pending token
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(t["bits"][2:], want[0][2:]) and bool((t["bits"][:2] == 0x5A5A5A5A).all())
    assert torch.equal(t["after"], want[2]) and torch.equal(t["safter"], want[4])


# ---------------- engine (llama3-8b-2l, captured graphs) ----------------
@pytest.fixture(scope="module")
def eng_be():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=4096, max_model_len=256))
    eng.runner.capture_graphs()
    return eng, EngineLLM(eng, max_new_tokens=8)


Q = "describe the pod as JSON"
FINITE = {"type": "object", "properties": {"ok": {"type": "boolean"}, "kind": {"enum": ["pod", "node", 7]},
                                           "flags": {"type": "array", "items": {"type": "boolean"}, "maxItems": 2}},
          "required": ["ok", "kind"]}
PAT = r"kubectl (get|describe) (pods|nodes|svc) -n [a-z0-9-]{1,6}"


def _text(eng, seq):
    tok = eng.tokenizer
    return tok.decode([t for t in seq.output_ids if not tok.is_eos(t)])


def _alone(eng, be, query, params):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params)[0]


def _valid_finite(v) -> bool:
    return isinstance(v, dict) and list(v) == [k for k in ("ok", "kind", "flags") if k in v] and "ok" in v \
        and "kind" in v and isinstance(v["ok"], bool) and v["kind"] in ("pod", "node", 7) \
        and all(isinstance(f, bool) for f in v.get("flags", [])) and len(v.get("flags", [])) <= 2


def test_engine_json_object_and_finite_schema(eng_be):
    eng, be = eng_be
    st = eng.runner.stats
    g = guided.compile_json_object()
    j0, g0 = st["json_steps"], st["guided_steps"]
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=False, guide=g))
    text = _text(eng, s)
    if s.finish_reason == "stop":
        assert isinstance(json.loads(text), dict), text
    else:
        assert s.finish_reason == "length" and g.is_prefix(text.encode()), text
    assert st["json_steps"] == j0 + len(s.output_ids) and st["guided_steps"] == g0 + len(s.output_ids)
    for seed in (1, 2):
        s = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=False, guide=g, temperature=1.0, seed=seed))
        text = _text(eng, s)
        assert g.is_prefix(text.encode()) and (s.finish_reason != "stop" or isinstance(json.loads(text), dict)), text
    f = guided.compile_json_schema(FINITE)
    for kw in (dict(), dict(temperature=1.0, seed=3), dict(temperature=1.5, seed=4)):
        s = _alone(eng, be, Q, SamplingParams(max_new_tokens=64, safe_decode=False, guide=f, **kw))
        assert s.finish_reason == "stop" and _valid_finite(json.loads(_text(eng, s))), _text(eng, s)
    assert s.guide_ref is None and all(p.refs == 0 for p in eng.runner.guide_table.placed.values())


def test_engine_logprobs_stay_inside_the_guide(eng_be):
    eng, be = eng_be
    tok = eng.tokenizer
    g = guided.compile_json_object()
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=16, safe_decode=False, guide=g, logprobs=20))
    assert len(s.logprobs) == len(s.generated) > 0
    state, stack = 0, ()
    for t, rec in zip(s.generated, s.logprobs):
        live = [i for i in rec.top_ids if i >= 0]
        for i in live:
            if tok.is_eos(i):
                assert g.accept[state]
            else:
                assert tok.token_bytes(i) and g.walk(state, tok.token_bytes(i), stack)[0] >= 0, (state, tok.token_bytes(i))
        assert t in live and np.isfinite(rec.logprob) and rec.logprob <= 0.0
        if not tok.is_eos(t):
            state, stack = g.walk(state, tok.token_bytes(t), stack)


def test_engine_same_bytes_in_mixed_company_and_plain_steps_stage_nothing(eng_be):
    from tests.guided_cases import chain_async
    from tests.test_guided_gpu import _run_sync
    eng, be = eng_be
    st = eng.runner.stats
    g, f, rx = guided.compile_json_object(), guided.compile_json_schema(FINITE), guided.compile_regex(PAT)
    pj = SamplingParams(max_new_tokens=24, safe_decode=False, guide=g, temperature=0.8, seed=5)
    pf = SamplingParams(max_new_tokens=64, safe_decode=False, guide=f)
    pr = SamplingParams(max_new_tokens=40, safe_decode=False, guide=rx)
    want_j, want_f, want_r = _alone(eng, be, Q, pj), _alone(eng, be, Q, pf), _alone(eng, be, Q, pr)
    eng.bm.reset_prefix_cache()
    assert chain_async(eng, Sequence(prompt_ids=be.prompt_ids(Q), params=pj)) == want_j.output_ids
    plain = dict(max_new_tokens=6, ignore_eos=True)
    eng.bm.reset_prefix_cache()
    staged = []
    orig = eng.runner._stage_guide_stacks
    eng.runner._stage_guide_stacks = lambda *a, **k: staged.append(1) or orig(*a, **k)
    try:
        j0, r0 = st["json_steps"], st["graph_replays"]
        ref_plain = eng.generate_blocking([be.prompt_ids("get nodes")], SamplingParams(**plain), forced_prefix=be._forced)[0]
        assert st["graph_replays"] == r0 + plain["max_new_tokens"] - 1
        again_r = _alone(eng, be, Q, pr)      # a regex-only step runs the old kernel on the old image
        assert again_r.output_ids == want_r.output_ids and not staged and st["json_steps"] == j0
    finally:
        eng.runner._stage_guide_stacks = orig
    # two-row steps (one- and two-row steps compute a row's logits alike: tests/test_penalties_gpu.py): a stack row
    # beside a DFA row in one launch of the stack kernel, and beside a plain row
    for want, p in ((want_j, pj), (want_f, pf)):
        pair = _run_sync(eng, [Sequence(prompt_ids=be.prompt_ids(Q), params=p),
                               Sequence(prompt_ids=be.prompt_ids(Q), params=pr)])
        assert pair[0].output_ids == want.output_ids and pair[1].output_ids == want_r.output_ids
        pair = _run_sync(eng, [Sequence(prompt_ids=be.prompt_ids(Q), params=p),
                               Sequence(prompt_ids=be.prompt_ids("get nodes"), params=SamplingParams(**plain),
                                        forced_prefix=list(be._forced))])
        assert pair[0].output_ids == want.output_ids and pair[1].output_ids == ref_plain.output_ids
    assert all(p.refs == 0 for p in eng.runner.guide_table.placed.values())
