"""csrc/guide_mask.hip (`ops.guide_mask`) against the literal pure-Python reference of tests/guided_cases.py, and
guided requests in the engine beside its captured greedy graphs.

Everything is integer, so every comparison is `torch.equal`: the whole bits tensor (the copied SAFE_DECODE rows,
the zero rows of requests that are not guided, the bits past V), idx and state_after, per case of
guided_cases (V around the word, the ballot and the workgroup tile and at 128256; 1, 3 and 64 rows; every
state kind, pending mode and base mode).  Then the launcher's return codes and the engine.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine import guided  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import guided_cases as gc  # noqa: E402

DEV = "cuda"
HIP_INVALID = 1   # hipErrorInvalidValue


@pytest.fixture(autouse=True, scope="module")
def _lib():
    lib = _hip.require()
    assert lib.ka_guide_mask_tile() == gc.TILE   # the geometry the cases straddle is the kernel's
    gc.check_preconditions()


def _want(c):
    bits, idx, after = gc.literal(c)
    return (torch.from_numpy(bits.view(np.int32).copy()).to(DEV), torch.from_numpy(idx.copy()).to(DEV),
            torch.from_numpy(after.copy()).to(DEV))


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_mask_matches_the_literal_reference_exactly(case):
    wb, wi, wa = _want(case)
    bits, idx, after = gc.run_ops(case, DEV)
    assert bits.shape == wb.shape and bits.dtype == torch.int32
    bad = (bits != wb).nonzero()
    assert torch.equal(bits, wb), (case.id, len(bad), bad[:5].tolist())
    assert torch.equal(idx, wi), (idx.tolist(), wi.tolist())
    assert torch.equal(after, wa), (after.tolist(), wa.tolist())
    again = gc.run_ops(case, DEV)
    assert torch.equal(again[0], bits) and torch.equal(again[1], idx) and torch.equal(again[2], after)


def test_launcher_refuses_invalid_arguments():
    lib = _hip.require()
    c = next(x for x in gc.CASES if x.V == 520 and x.rows == 3 and x.base_bits is not None and x.pend_src is not None)
    tb = gc.token_table(c.V, DEV)

    def dev(a, view=None):
        return torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view))).to(DEV)

    words = (c.V + 31) // 32
    t = dict(bits=torch.zeros((2 + c.rows, words), dtype=torch.int32, device=DEV),
             idx=torch.zeros(c.rows, dtype=torch.int32, device=DEV),
             after=torch.zeros(c.rows, dtype=torch.int32, device=DEV), rec=tb.rec, ovf=tb.ovf,
             arena=dev(c.trans, np.int16), accept=dev(c.accept), base=dev(c.row_base), nst=dev(c.row_nstates),
             st=dev(c.row_state), pend=dev(c.pend_src), tokens=dev(c.tokens), bbits=dev(c.base_bits, np.int32),
             bidx=dev(c.base_idx))
    good = dict(ovf_bytes=tb.ovf_bytes, vocab=c.V, eos0=c.eos_ids[0], arena_states=c.trans.shape[0],
                n_tokens=len(c.tokens), n_static=2, rows=c.rows)

    def call(**kw):
        a = {k: v.data_ptr() for k, v in t.items()}
        a.update(good)
        a.update(kw)
        return lib.ka_guide_mask(a["bits"], a["idx"], a["after"], a["rec"], a["ovf"], a["ovf_bytes"], a["vocab"],
                                 a["eos0"], a["arena"], a["accept"], a["arena_states"], a["base"], a["nst"], a["st"],
                                 a["pend"], a["tokens"], a["n_tokens"], a["bbits"], a["bidx"], a["n_static"], a["rows"],
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    want = _want(c)[0][2:]   # the launcher writes the batch rows; ops.guide_mask copies the SAFE_DECODE rows in front
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(t["bits"][2:], want)
    t["bits"].fill_(0x5A5A5A5A)
    bad = [dict(bits=None), dict(idx=None), dict(after=None), dict(rec=None), dict(arena=None), dict(accept=None),
           dict(base=None), dict(nst=None), dict(st=None), dict(tokens=None), dict(bbits=None), dict(bidx=None),
           dict(ovf=None), dict(n_static=0), dict(bbits=None, bidx=None), dict(rec=t["rec"].data_ptr() + 4),
           dict(rows=-1), dict(rows=65536), dict(vocab=0), dict(vocab=-5), dict(eos0=-1), dict(eos0=c.V),
           dict(arena_states=0), dict(ovf_bytes=-1), dict(n_tokens=-1), dict(n_static=-1)]
    assert tb.ovf_bytes > 0
    for kw in bad:
        assert call(**kw) == HIP_INVALID, kw
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert bool((t["bits"] == 0x5A5A5A5A).all())   # none of them launched anything
    assert call(pend=None, tokens=None, n_tokens=0) == 0      # no row has a pending token
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(t["bits"][2:], want) and bool((t["bits"][:2] == 0x5A5A5A5A).all())


# ---------------- engine (llama3-8b-2l, captured graphs) ----------------
@pytest.fixture(scope="module")
def eng_be():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=4096, max_model_len=256))
    eng.runner.capture_graphs()
    return eng, EngineLLM(eng, max_new_tokens=8)


PAT = r"kubectl (get|describe) (pods|nodes|svc) -n [a-z0-9-]{1,6}"
CHOICES = ["pods", "nodes", "services", "deployments"]
Q = "list pods in prod"


def _text(eng, seq):
    tok = eng.tokenizer
    return tok.decode([t for t in seq.output_ids if not tok.is_eos(t)])


def _alone(eng, be, query, params):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params)[0]


def test_engine_match_and_prefix(eng_be):
    eng, be = eng_be
    g, gch = guided.compile_regex(PAT), guided.compile_choice(CHOICES)
    st = eng.runner.stats
    before = st["guided_steps"]
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=40, safe_decode=False, guide=g))
    assert s.finish_reason == "stop" and re.fullmatch(PAT, _text(eng, s)), _text(eng, s)
    assert st["guided_steps"] == before + len(s.output_ids)
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=40, safe_decode=False, guide=gch))
    assert s.finish_reason == "stop" and _text(eng, s) in CHOICES
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=3, safe_decode=False, guide=g))
    assert s.finish_reason == "length" and len(s.output_ids) == 3
    assert g.is_prefix(_text(eng, s).encode()) and not g.matches(_text(eng, s).encode())


def _run_sync(eng, seqs):
    """Step `seqs` (each with its own parameters) through the synchronous path, admitted together."""
    eng.bm.reset_prefix_cache()
    sch = eng.scheduler
    saved = (sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps)
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    try:
        for s in seqs:
            sch.add(s)
        while any(not s.finished for s in seqs):
            batch = sch.schedule()
            eng._apply(batch, eng.runner.execute(batch))
            sch.on_step_done(batch)
    finally:
        sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = saved
    return seqs


def test_engine_seed_reproducible_and_batch_independent(eng_be):
    """A guided request returns the same bytes alone, chained behind tokens still on the device and in two-row
    batches beside a greedy, a sampled and a penalised request, and each companion returns what it returns
    alone (one- and two-row steps compute a row's logits alike on the GPU: tests/test_penalties_gpu.py).  Plain
    batches replay their graphs and count no guided step."""
    import threading
    from ai_agent_kubectl_amd.engine.sequence import Sequence
    eng, be = eng_be
    g = guided.compile_regex(PAT)
    pg = SamplingParams(max_new_tokens=40, safe_decode=False, guide=g)
    ps = SamplingParams(max_new_tokens=40, safe_decode=False, guide=g, temperature=0.9, seed=11)
    want_g, want_s = _alone(eng, be, Q, pg), _alone(eng, be, Q, ps)
    assert re.fullmatch(PAT, _text(eng, want_s)) and _alone(eng, be, Q, ps).output_ids == want_s.output_ids
    # chained: every decode step's state is completed on the device from the token still in d_out
    eng.bm.reset_prefix_cache()
    assert gc.chain_async(eng, Sequence(prompt_ids=be.prompt_ids(Q), params=ps)) == want_s.output_ids
    st = eng.runner.stats
    others = [("get nodes -o wide", dict(max_new_tokens=6, ignore_eos=True)),
              ("describe pod web-1", dict(max_new_tokens=5, ignore_eos=True, temperature=0.7, seed=3)),
              ("top nodes", dict(max_new_tokens=6, ignore_eos=True, frequency_penalty=2.0))]
    for q, kw in others:
        eng.bm.reset_prefix_cache()
        g0, r0 = st["guided_steps"], st["graph_replays"]
        ref_run = eng.generate_blocking([be.prompt_ids(q)], SamplingParams(**kw), forced_prefix=be._forced)[0]
        assert st["guided_steps"] == g0
        if len(kw) == 2:   # the plain request: one prefill, then every decode step a graph replay
            assert st["graph_replays"] == r0 + kw["max_new_tokens"] - 1
        for want, p in ((want_g, pg), (want_s, ps)):
            pair = _run_sync(eng, [Sequence(prompt_ids=be.prompt_ids(Q), params=p),
                                   Sequence(prompt_ids=be.prompt_ids(q), params=SamplingParams(**kw),
                                            forced_prefix=list(be._forced))])
            assert pair[0].output_ids == want.output_ids, q
            assert pair[1].output_ids == ref_run.output_ids, q
    # the threaded engine with lookahead: the guided requests still match, and every placement is released
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == 3:
            ev.set()

    eng.start()
    try:
        a = eng.submit(be.prompt_ids("get nodes -o wide"), SamplingParams(**others[0][1]), cb, forced_prefix=be._forced)
        b = eng.submit(be.prompt_ids(Q), pg, cb)
        c = eng.submit(be.prompt_ids("list the nodes"), ps, cb)
        assert ev.wait(120)
    finally:
        eng.shutdown()
    assert eng.healthy and a.num_generated == 6
    for s in (b, c):
        assert s.finish_reason == "stop" and re.fullmatch(PAT, _text(eng, s)), _text(eng, s)
    assert b.guide_ref is None and all(p.refs == 0 for p in eng.runner.guide_table.placed.values())
