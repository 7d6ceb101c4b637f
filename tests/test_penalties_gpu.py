"""csrc/logit_adjust.hip (`ops.logit_adjust` / `ops.logit_restore`) against the literal numpy formula of
tests/penalty_cases.py, and the engine's penalty steps beside its captured greedy graphs.

Every comparison is exact: `torch.equal` on the int16 view of the whole [R, V] tensor, which also shows
that no logit without an entry moved.  Per geometry case (penalty_cases: the sampler's V / R / offsets,
entries per row around the workgroup size and the per-thread batch, ids at both ends of the slice and
outside it, runs of consecutive ids, neutral rows between active ones, every pending-token mode):
* adjust == reference, with and without the saved patterns; the saved slots == the reference's;
* restore after adjust == the original bits; two launches from the same input give the same bits.
Then the pending token by hand, the launcher's return codes and the engine.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import penalty_cases as pc  # noqa: E402
from tests import sampling_cases as sc  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _lib():
    lib = _hip.require()
    # the geometry the cases straddle is the kernel's
    assert lib.ka_logit_adjust_threads() == pc.NT and lib.ka_logit_adjust_batch() == pc.BATCH


def _adjust(t, save=False, pend=True):
    return ops.logit_adjust(t["logits"], t["row_start"], t["ent_id"], t["ent_cnt"], t["ent_bias"], t["presence"],
                            t["frequency"], t["repetition"], t["pend_src"] if pend else None,
                            t["tokens"] if pend else None, vocab_offset=t["off"], save=save)


def _restore(t, saved):
    ops.logit_restore(t["logits"], t["row_start"], t["ent_id"], t["presence"], t["frequency"], t["repetition"],
                      t["pend_src"], t["tokens"], saved, vocab_offset=t["off"])


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_adjust_and_restore_match_the_reference_exactly(case):
    inp, want = pc.build(case)
    t = dict(pc.as_torch(inp, DEV), off=inp["off"])
    saved = _adjust(t, save=True)
    got = pc.bits(t["logits"])
    wl = pc.want_bits(want["logits"])
    bad = (got != wl).nonzero()
    assert torch.equal(got, wl), (pc.case_id(case), len(bad), bad[:5].tolist())
    assert saved.shape == (case[1] + len(inp["ent_id"]),) and saved.dtype == BF
    assert torch.equal(pc.bits(saved), pc.want_bits(want["saved"])), "saved slots"
    _restore(t, saved)
    assert torch.equal(pc.bits(t["logits"]), pc.want_bits(inp["logits"])), "restore"
    # a second launch from the same input, this time without saving: the same bits
    t2 = dict(pc.as_torch(inp, DEV), off=inp["off"])
    assert _adjust(t2) is None
    assert torch.equal(pc.bits(t2["logits"]), got)


def test_pending_token_modes():
    """By hand at V = 520 (one row of entries, one empty row, one neutral row): absent; matching the first,
    the last and a middle entry; no entry has it; on the row with the empty segment; another row's slot."""
    V, off, R = 520, 64, 3
    n = 300   # more than one workgroup's worth of threads: entry 299 is thread 43's second
    rs = np.random.RandomState(5)
    ids = (rs.permutation(V)[:n] + off).astype(np.int32)
    free = np.setdiff1d(np.arange(off, off + V), ids)
    base = dict(row_start=np.array([0, n, n, n], dtype=np.int32), ent_id=ids,
                ent_cnt=rs.randint(0, 4, size=n).astype(np.int32), ent_bias=np.zeros(n, dtype=np.float32),
                presence=np.array([0.5, 1.0, 0.0], dtype=np.float32), frequency=np.array([0.25, 0.5, 0.0], dtype=np.float32),
                repetition=np.array([1.0, 1.5, 1.0], dtype=np.float32), logits=pc.make_logits(R, V, 77))
    for name, pend_src, tokens in (("absent", [-1, -1, -1], [ids[0], ids[0], ids[0], 0]),
                                   ("first", [0, -1, -1], [ids[0], 0, 0, 0]),
                                   ("last", [0, -1, -1], [ids[-1], 0, 0, 0]),
                                   ("middle", [0, -1, -1], [ids[n // 2], 0, 0, 0]),
                                   ("no entry", [0, -1, -1], [free[3], 0, 0, 0]),
                                   ("empty segment", [-1, 1, 2], [0, free[5], free[6], 0]),
                                   ("another row's slot", [3, 0, -1], [free[1], 0, 0, ids[7]]),
                                   ("past the token array", [4, -1, -1], [ids[0], 0, 0, 0])):
        inp = dict(base, pend_src=np.array(pend_src, dtype=np.int32), tokens=np.array(tokens, dtype=np.int32), off=off)
        want, wsaved, _ = pc.np_reference(inp["logits"], inp["row_start"], inp["ent_id"], inp["ent_cnt"], inp["ent_bias"],
                                          inp["presence"], inp["frequency"], inp["repetition"], inp["pend_src"],
                                          inp["tokens"], off)
        t = dict(pc.as_torch(inp, DEV), off=off)
        saved = _adjust(t, save=True)
        assert torch.equal(pc.bits(t["logits"]), pc.want_bits(want)), name
        assert torch.equal(pc.bits(saved), pc.want_bits(wsaved)), name
        changed = (want != inp["logits"]).sum(axis=1)
        assert changed[2] == 0, name                      # the neutral row: untouched whatever it is handed
        if name == "empty segment":
            assert changed[1] == 1 and saved[1].view(torch.int16).item() == pc.want_bits(inp["logits"])[1, free[5] - off].item()
        _restore(t, saved)
        assert torch.equal(pc.bits(t["logits"]), pc.want_bits(inp["logits"])), name
    # no pend_src at all is the same as all -1
    inp = dict(base, pend_src=np.full(R, -1, dtype=np.int32), tokens=np.zeros(4, dtype=np.int32), off=off)
    a, b = dict(pc.as_torch(inp, DEV), off=off), dict(pc.as_torch(inp, DEV), off=off)
    _adjust(a)
    _adjust(b, pend=False)
    assert torch.equal(pc.bits(a["logits"]), pc.bits(b["logits"]))


def test_launcher_return_codes():
    lib = _hip.require()
    p = ops._p
    R, V, E = 2, 16, 3
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)      # noqa: E731
    f32 = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)    # noqa: E731
    logits = torch.zeros(R, V, dtype=BF, device=DEV)
    rs, ids, cnt, bias = i32(0, 2, 3), i32(1, 2, 3), i32(1, 0, 2), f32(0.0, 1.0, 0.0)
    pres, freq, rep, pend, tok = f32(0.5, 0.0), f32(0.0, 0.5), f32(1.0, 1.0), i32(-1, 0), i32(5, 5)
    saved = torch.zeros(R + E, dtype=BF, device=DEV)
    st = ops._stream()
    good = [p(logits), p(rs), p(ids), p(cnt), p(bias), p(pres), p(freq), p(rep), p(pend), p(tok), 2, p(saved), R, E, V, 0, st]
    assert lib.ka_logit_adjust(*good) == 0
    for missing in (0, 1, 2, 3, 4, 5, 6, 7, 9):   # everything but pend_src and saved is required
        a = list(good)
        a[missing] = None
        assert lib.ka_logit_adjust(*a) == 1, missing
    for opt in (8, 11):                           # pend_src (with its tokens) and saved are optional
        a = list(good)
        a[opt] = None
        assert lib.ka_logit_adjust(*a) == 0, opt
    for pos, val in ((12, -1), (14, 0), (14, -8), (13, -1), (10, -1)):   # rows, vocab, entries, n_tokens
        a = list(good)
        a[pos] = val
        assert lib.ka_logit_adjust(*a) == 1, (pos, val)
    a = list(good)
    a[12] = 0                                     # no rows: success, nothing launched
    logits.zero_()
    torch.cuda.synchronize()
    assert lib.ka_logit_adjust(*a) == 0
    torch.cuda.synchronize()
    assert not bool(pc.bits(logits).any())
    assert lib.ka_logit_adjust(*good) == 0        # row 0: tokens 1 and 2; row 1: token 3 and the pending token 5
    torch.cuda.synchronize()
    assert (pc.bits(logits) != 0).nonzero().tolist() == [[0, 1], [0, 2], [1, 3], [1, 5]]
    rgood = [p(logits), p(rs), p(ids), p(pres), p(freq), p(rep), p(pend), p(tok), 2, p(saved), R, E, V, 0, st]
    assert lib.ka_logit_restore(*rgood) == 0
    for missing in (0, 1, 2, 3, 4, 5, 7, 9):      # restore needs the saved patterns
        a = list(rgood)
        a[missing] = None
        assert lib.ka_logit_restore(*a) == 1, missing
    for pos, val in ((10, -1), (12, 0), (11, -1)):
        a = list(rgood)
        a[pos] = val
        assert lib.ka_logit_restore(*a) == 1, (pos, val)
    a = list(rgood)
    a[10] = 0
    assert lib.ka_logit_restore(*a) == 0
    torch.cuda.synchronize()
    assert not bool(pc.bits(logits).any())        # adjust, then restore
    # the Python wrappers check what the launcher cannot
    with pytest.raises(ValueError):
        ops.logit_adjust(logits.float(), rs, ids, cnt, bias, pres, freq, rep)
    with pytest.raises(ValueError):
        ops.logit_adjust(logits, rs[:2], ids, cnt, bias, pres, freq, rep)
    with pytest.raises(ValueError):
        ops.logit_adjust(logits, rs, ids, cnt[:2], bias, pres, freq, rep)
    with pytest.raises(ValueError):
        ops.logit_adjust(logits, rs, ids, cnt, bias, pres, freq, rep, pend_src=pend)
    with pytest.raises(ValueError):
        ops.logit_restore(logits, rs, ids, pres, freq, rep, pend, tok, saved[:2])


# ---------------- engine ----------------
@pytest.fixture(scope="module")
def eng_be():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    # llama3-8b-2l: the smallest preset the device kernels take; buckets 1 and 2 are the persistent decode
    # kernel's, 4 the kernel chain's
    eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=4096, max_model_len=256))
    eng.runner.capture_graphs()
    return eng, EngineLLM(eng, max_new_tokens=8)


Q = "list pods in prod"
N = 8


def _alone(eng, be, query, params, forced=True):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params, forced_prefix=be._forced if forced else None)[0]


def test_engine_bias_forces_a_token(eng_be):
    """(a) on the GPU, beside the captured graphs."""
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    eng, be = eng_be
    st, tok = eng.runner.stats, eng.tokenizer
    assert eng.runner.graphs
    before = st["penalty_steps"]
    t = next(i for i in range(1000, 2000) if not tok.is_eos(i))
    a = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, safe_decode=False, logit_bias={t: 100.0}), forced=False)
    assert a.output_ids == [t] * N and a.finish_reason == "length" and st["penalty_steps"] == before + N
    # a greedy-only run afterwards replays the graphs and counts no penalty step
    n2, r2 = st["penalty_steps"], st["graph_replays"]
    g = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True))
    assert st["graph_replays"] > r2 and st["penalty_steps"] == n2 and len(g.output_ids) == len(a.output_ids) + 1


def _run_sync(eng, seqs, preempt_at=-1):
    """Step `seqs` (each with its own parameters) through the synchronous path; preempt_at: the step before
    which seqs[0] is preempted (recomputed from prompt + outputs when re-admitted)."""
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
                assert seqs[0] in sch.running and seqs[0].num_generated == preempt_at
                sch._preempt(seqs[0])
            batch = sch.schedule()
            eng._apply(batch, eng.runner.execute(batch))
            sch.on_step_done(batch)
            step += 1
    finally:
        sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = saved
    return seqs


def _penalised(eng, be):
    """The request of (c): seeded sampling with all four fields, its bias aimed at what the same request
    generates without them, so that the fields decide the completion."""
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    base = dict(max_new_tokens=N, ignore_eos=True, temperature=0.9, top_k=50, seed=7)
    plain = _alone(eng, be, Q, SamplingParams(**base))
    kw = dict(base, presence_penalty=0.5, frequency_penalty=1.2, repetition_penalty=1.3,
              logit_bias={plain.generated[2]: -100.0, plain.generated[0]: -0.5, 2000: 4.0})
    return plain, kw


OTHERS = [("get nodes -o wide", dict(max_new_tokens=N, ignore_eos=True)),
          ("top nodes", dict(max_new_tokens=6, ignore_eos=True, frequency_penalty=2.0, logprobs=2)),
          ("describe pod web-1", dict(max_new_tokens=5, ignore_eos=True, temperature=0.7, seed=3))]


def test_engine_same_tokens_through_every_launch_path(eng_be):
    """(c) on the GPU: alone and synchronous, chained behind tokens still on the device, and inside two-row
    batches beside a greedy, a penalised logprobs and a sampled request; each companion returns what it
    returns alone.  The request samples (T = 0.9, top_k 50, seed 7) with all four fields.  (One- and two-row
    steps compute a row's logits alike on the GPU; larger buckets and recomputed KV do not, see the next test.)"""
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    eng, be = eng_be
    plain, kw = _penalised(eng, be)
    want = _alone(eng, be, Q, SamplingParams(**kw))
    assert _alone(eng, be, Q, SamplingParams(**kw)).output_ids == want.output_ids
    assert want.output_ids != plain.output_ids and plain.generated[2] not in want.output_ids
    assert -1 not in want.output_ids
    # chained: the newest token of every decode step is counted on the device
    eng.bm.reset_prefix_cache()
    assert sc.chain_async(eng, sc.new_sequence(be, Q, SamplingParams(**kw))) == want.output_ids
    for q, okw in OTHERS:
        ref_run = _alone(eng, be, q, SamplingParams(**okw))
        pair = _run_sync(eng, [sc.new_sequence(be, Q, SamplingParams(**kw)), sc.new_sequence(be, q, SamplingParams(**okw))])
        assert pair[0].output_ids == want.output_ids, q
        assert pair[1].output_ids == ref_run.output_ids, q   # a request beside a penalised one: what it returns alone
        assert len(pair[1].logprobs) == len(ref_run.logprobs)


class _Recorder:
    """Stands in for ops.logit_adjust during a run: every launch's inputs, and whether it edited the step's
    logits exactly as the reference does from the same inputs."""

    def __init__(self):
        self.calls, self.orig = [], ops.logit_adjust

    def __enter__(self):
        ops.logit_adjust = self
        return self

    def __exit__(self, *exc):
        ops.logit_adjust = self.orig

    def __call__(self, logits, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src=None,
                 tokens=None, vocab_offset=0, save=False):
        # device clones only, queued on the step's stream: nothing here waits for the GPU, so the engine's
        # lookahead overlaps as it does in service; check() compares after the run
        args = [t.clone() for t in (row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src, tokens)]
        before = logits.clone()
        out = self.orig(logits, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src, tokens,
                        vocab_offset=vocab_offset, save=save)
        self.calls.append(dict(args=args, before=before, after=logits.clone(), off=vocab_offset))
        return out

    def check(self, finals):
        """finals: {repetition_penalty: the output_ids that request went on to return}.  Every launch was
        exact, and per penalised row the counts it was handed plus the pending token read on the device are
        the Counter of a prefix of those outputs.  -> (launches per request, rows with a pending token)."""
        from collections import Counter
        from ai_agent_kubectl_amd.ops import reference as ref
        torch.cuda.synchronize()
        assert self.calls
        per_request, pending, moved = Counter(), 0, 0
        for c in self.calls:
            c["args"] = [t.cpu() for t in c["args"]]
            expect = c["before"].cpu()
            ref.logit_adjust(expect, *c["args"], vocab_offset=c["off"])
            assert torch.equal(pc.bits(c["after"]), pc.bits(expect)), "a launch edited the logits otherwise than the reference"
            moved += int((pc.bits(expect) != pc.bits(c["before"])).sum())
            row_start, ent_id, ent_cnt, _, presence, frequency, repetition, pend_src, tokens = c["args"]
            rs = row_start.tolist()
            for r in range(len(rs) - 1):
                if (float(presence[r]), float(frequency[r]), float(repetition[r])) == (0.0, 0.0, 1.0):
                    assert rs[r] == rs[r + 1] and int(pend_src[r]) == -1   # a row without the fields: nothing to do
                    continue
                key = round(float(repetition[r]), 4)
                cnt = Counter()
                for t, w in zip(ent_id[rs[r]:rs[r + 1]].tolist(), ent_cnt[rs[r]:rs[r + 1]].tolist()):
                    if w & 0x7FFFFFFF:
                        cnt[t] += w & 0x7FFFFFFF
                if int(pend_src[r]) >= 0:
                    pending += 1
                    cnt[int(tokens[int(pend_src[r])])] += 1
                n = sum(cnt.values())
                assert cnt == Counter(finals[key][:n]), (r, n)
                per_request[key] += 1
        assert moved > 0
        return per_request, pending


def _deterministic(eng, be):
    """The request of (c) for the conditions whose arithmetic differs from the alone-run's: all four fields at
    temperature 0 (the seed is carried and ignored), the bias aimed at what the request returns without them.
    Its choice is the masked argmax of the edited logits and does not hang on a Gumbel near-tie."""
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    base = dict(max_new_tokens=N, ignore_eos=True, temperature=0.0, seed=7)
    plain = _alone(eng, be, Q, SamplingParams(**base))
    kw = dict(base, presence_penalty=1.0, frequency_penalty=1.5, repetition_penalty=1.5,
              logit_bias={plain.generated[2]: -100.0, plain.generated[0]: -0.5, 2000: 4.0})
    return plain, kw


def test_engine_same_tokens_across_a_preemption_and_in_a_threaded_mixed_batch(eng_be):
    """(c) across a forced preemption and in the threaded engine with lookahead and four mixed requests: the
    same penalised request returns the tokens of its alone-run.
    On the GPU these two conditions do not compute a row's logits as the alone-run does: a preempted request's
    KV is recomputed by the prefill kernels, and a four-row bucket or a mixed step runs other GEMM kernels.
    The SAMPLED request of the test above, WITHOUT penalties, already leaves its alone-run there
    (scripts/diag_penalty_paths.py, profiles/penalties/diag_*.log), so these conditions are asserted with the
    temperature-0 request of `_deterministic`.  In addition every adjust launch of both runs is checked: the
    counts it was handed plus the pending token read on the device are exactly the Counter of the tokens the
    request went on to return, also after the recompute, and the launch edited the step's logits exactly as
    the reference does."""
    import threading
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    eng, be = eng_be
    plain, kw = _deterministic(eng, be)
    want = _alone(eng, be, Q, SamplingParams(**kw))
    assert want.output_ids != plain.output_ids and plain.generated[2] not in want.output_ids
    eng.bm.reset_prefix_cache()
    assert sc.chain_async(eng, sc.new_sequence(be, Q, SamplingParams(**kw))) == want.output_ids
    # a forced preemption after four tokens, beside a greedy request
    q, okw = OTHERS[0]
    g_alone = _alone(eng, be, q, SamplingParams(**okw))
    with _Recorder() as rec:
        pair = _run_sync(eng, [sc.new_sequence(be, Q, SamplingParams(**kw)), sc.new_sequence(be, q, SamplingParams(**okw))],
                         preempt_at=4)
    assert pair[0].output_ids == want.output_ids
    assert pair[1].output_ids == g_alone.output_ids
    per_request, _ = rec.check({1.5: pair[0].output_ids})
    assert per_request[1.5] == N   # the recomputing prefill is the launch of the fifth token: none twice, none missing
    # the threaded engine
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == 4:
            ev.set()

    n0 = eng.lookahead_steps
    with _Recorder() as rec:
        eng.start()
        try:
            got = [eng.submit(be.prompt_ids(x), SamplingParams(**p), cb, forced_prefix=be._forced)
                   for x, p in [("get svc -A", dict(max_new_tokens=3, ignore_eos=True)), (Q, kw)] + OTHERS[1:]]
            assert ev.wait(60)
        finally:
            eng.shutdown()
    assert eng.healthy and eng.lookahead_steps > n0
    assert all(len(s.output_ids) == s.params.max_new_tokens + 1 and -1 not in s.output_ids for s in got)
    assert len(got[2].logprobs) == 6
    per_request, pending = rec.check({1.5: got[1].output_ids, 1.0: got[2].output_ids})
    # every generated token of both penalised requests went through one launch, most with a token still pending
    assert per_request[1.5] == N and per_request[1.0] == 6 and pending >= N
    assert got[1].output_ids == want.output_ids


def test_engine_logprobs_stay_the_raw_ones(eng_be):
    """(d) on the GPU."""
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    eng, be = eng_be
    free = dict(max_new_tokens=N, ignore_eos=True, safe_decode=False)
    raw = _alone(eng, be, Q, SamplingParams(**free, logprobs=20), forced=False)
    t = next(i for i in range(1000, 2000) if i not in raw.logprobs[0].top_ids)
    pen = _alone(eng, be, Q, SamplingParams(**free, logprobs=20, logit_bias={t: 100.0}, frequency_penalty=0.5), forced=False)
    assert pen.output_ids == [t] * N and len(pen.logprobs) == N
    assert pen.logprobs[0].top_ids == raw.logprobs[0].top_ids
    assert pen.logprobs[0].top_logprobs == raw.logprobs[0].top_logprobs
    for rec in pen.logprobs:
        assert t not in rec.top_ids and np.isfinite(rec.logprob) and rec.logprob <= rec.top_logprobs[-1] < 0.0
    # the chosen token's record is its raw value in the top list whenever it is there
    g = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True, logprobs=20, frequency_penalty=2.0,
                                          presence_penalty=2.0, repetition_penalty=1.5))
    for tok, rec in zip(g.generated, g.logprobs):
        if tok in rec.top_ids:
            assert rec.logprob == rec.top_logprobs[rec.top_ids.index(tok)]
        else:
            assert rec.logprob <= rec.top_logprobs[-1]
