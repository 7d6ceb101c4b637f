"""presence / frequency / repetition penalties and logit_bias on the CPU: the reference's definition
(ops/reference.py `logit_adjust`, against the literal numpy formula of tests/penalty_cases.py), the host
packer (engine/penalties.py, against a collections.Counter oracle), the engine on tiny-llama through every
launch path, and the /v1/chat/completions fields.  The HIP kernel is in test_penalties_gpu.py."""
import threading

import numpy as np
import pytest
import torch

from ai_agent_kubectl_amd import ops
from ai_agent_kubectl_amd.engine import penalties
from ai_agent_kubectl_amd.engine.sequence import PLACEHOLDER, SamplingParams, Sequence
from ai_agent_kubectl_amd.models.llama import LogitEdits
from tests import penalty_cases as pc
from tests import sampling_cases as sc

BF = torch.bfloat16


# ---------------- the reference ----------------
def _adjust(t, save=False, pend=True):
    return ops.logit_adjust(t["logits"], t["row_start"], t["ent_id"], t["ent_cnt"], t["ent_bias"], t["presence"],
                            t["frequency"], t["repetition"], t["pend_src"] if pend else None,
                            t["tokens"] if pend else None, vocab_offset=t["off"], save=save)


def _restore(t, saved):
    ops.logit_restore(t["logits"], t["row_start"], t["ent_id"], t["presence"], t["frequency"], t["repetition"],
                      t["pend_src"], t["tokens"], saved, vocab_offset=t["off"])


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[0] <= 32776], ids=pc.case_id)
def test_torch_reference_is_the_literal_formula(case):
    inp, want = pc.build(case)
    t = dict(pc.as_torch(inp), off=inp["off"])
    saved = _adjust(t, save=True)
    assert torch.equal(pc.bits(t["logits"]), pc.want_bits(want["logits"]))
    assert saved.dtype == BF and torch.equal(pc.bits(saved), pc.want_bits(want["saved"]))
    _restore(t, saved)
    assert torch.equal(pc.bits(t["logits"]), pc.want_bits(inp["logits"]))
    # without saving: the same logits, nothing returned
    t = dict(pc.as_torch(inp), off=inp["off"])
    assert _adjust(t) is None and torch.equal(pc.bits(t["logits"]), pc.want_bits(want["logits"]))


def _one(logit, c=0, prompt=False, bias=0.0, presence=0.0, frequency=0.0, repetition=1.0, V=16, at=5):
    """The formula through ops.logit_adjust on a one-row tensor of zeros with `logit` at `at` -> that value."""
    l = torch.zeros(1, V, dtype=BF)
    l[0, at] = logit
    before = l.clone()
    ops.logit_adjust(l, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([at], dtype=torch.int32),
                     torch.tensor([c | (pc.PROMPT_BIT if prompt else 0)], dtype=torch.int64).to(torch.int32),
                     torch.tensor([bias]), torch.tensor([presence]), torch.tensor([frequency]), torch.tensor([repetition]))
    keep = torch.arange(V) != at
    assert torch.equal(pc.bits(l)[0, keep], pc.bits(before)[0, keep])   # no other logit moved
    return float(l[0, at])


def test_reference_properties():
    # repetition at a positive, a negative and a zero logit; only for a token that was seen
    assert _one(3.0, c=1, repetition=1.5) == 2.0 and _one(-3.0, c=1, repetition=1.5) == -4.5
    assert _one(0.0, c=1, repetition=1.5) == 0.0
    assert _one(3.0, prompt=True, repetition=1.5) == 2.0          # the prompt counts as seen
    assert _one(3.0, repetition=1.5, bias=0.0) == 3.0             # an entry that was never seen
    assert _one(3.0, c=2, repetition=0.5) == 6.0 and _one(-3.0, c=2, repetition=0.5) == -1.5
    # c = 0, 1 and 7: frequency times c, presence once
    for c, want in ((0, 4.0), (1, 4.0 - 0.5 - 0.25), (7, 4.0 - 3.5 - 0.25)):
        assert _one(4.0, c=c, frequency=0.5, presence=0.25) == want
    assert _one(4.0, prompt=True, frequency=0.5, presence=0.25) == 4.0   # the prompt alone: no count
    assert _one(1.0, c=3, frequency=-2.0, presence=-2.0) == 9.0
    # -inf stays -inf; bias +-100
    for kw in (dict(c=3, frequency=2.0, presence=2.0, repetition=2.0, bias=100.0), dict(bias=-100.0), dict(c=1, repetition=0.5)):
        assert _one(float("-inf"), **kw) == float("-inf")
    assert _one(2.5, bias=100.0) == 102.5 and _one(2.5, bias=-100.0) == -97.5
    # the order: repetition, frequency, presence, bias
    assert _one(8.0, c=2, repetition=2.0, frequency=0.5, presence=1.0, bias=0.25) == ((8.0 / 2 - 1.0) - 1.0) + 0.25
    # the result is bf16: below half an ulp of the logit (0.0625 at magnitude 16-32) nothing changes
    assert _one(20.0, bias=0.05) == 20.0 and _one(20.0, bias=0.07) == 20.125
    assert _one(20.0, c=1, frequency=0.0625) == 20.0   # exactly half an ulp: ties to even


def test_neutral_parameters_and_no_bias_leave_every_bit_unchanged():
    inp, _ = pc.build((520, 64, 64))
    t = dict(pc.as_torch(inp), off=64)
    # rows without entries (the packer's rows for requests without the fields), with or without a pending token
    t["row_start"] = torch.zeros_like(t["row_start"])
    for k, v in (("presence", 0.0), ("frequency", 0.0), ("repetition", 1.0)):
        t[k] = torch.full_like(t[k], v)
    assert (inp["logits"] == 0x8000).any()   # a -0 among them
    saved = _adjust(t, save=True)
    assert torch.equal(pc.bits(t["logits"]), pc.want_bits(inp["logits"])) and not bool(pc.bits(saved).any())
    # entries with neutral parameters and zero bias: equal values everywhere (a touched -0 reads +0)
    t = dict(pc.as_torch(inp), off=64)
    for k, v in (("presence", 0.0), ("frequency", 0.0), ("repetition", 1.0)):
        t[k] = torch.full_like(t[k], v)
    t["ent_bias"] = torch.zeros_like(t["ent_bias"])
    _adjust(t)
    got, was = pc.bits(t["logits"]), pc.want_bits(inp["logits"])
    diff = got != was
    assert bool((was[diff] == -0x8000).all()) and bool((got[diff] == 0).all())   # int16 views: -0 is -0x8000


def test_pending_token_counts_once():
    V = 32
    base = dict(row_start=torch.tensor([0, 2, 2], dtype=torch.int32), ent_id=torch.tensor([4, 9], dtype=torch.int32),
                ent_cnt=torch.tensor([2, 0], dtype=torch.int32), ent_bias=torch.tensor([0.0, 1.0]),
                presence=torch.tensor([0.5, 0.5]), frequency=torch.tensor([1.0, 1.0]), repetition=torch.tensor([1.0, 1.0]))

    def run(pend_src, tokens):
        l = torch.full((2, V), 8.0, dtype=BF)
        ops.logit_adjust(l, **base, pend_src=torch.tensor(pend_src, dtype=torch.int32),
                         tokens=torch.tensor(tokens, dtype=torch.int32))
        return l.float()

    l = run([-1, -1], [4, 4, 4])
    assert l[0, 4] == 8 - 2 - 0.5 and l[0, 9] == 9 and float(l[1].min()) == 8 == float(l[1].max())
    l = run([0, -1], [4, 7, 7])          # matches the first entry: c = 3
    assert l[0, 4] == 8 - 3 - 0.5 and l[0, 9] == 9
    l = run([2, 1], [0, 6, 9])           # another row's slot; matches the bias entry: c = 1; row 1: empty segment
    assert l[0, 9] == 8 - 1 - 0.5 + 1 and l[0, 4] == 8 - 2 - 0.5 and l[1, 6] == 8 - 1 - 0.5
    assert int((l[1] != 8).sum()) == 1 and int((l[0] != 8).sum()) == 2
    l = run([1, -1], [0, 20, 0])         # no entry has it: one more entry with c = 1
    assert l[0, 20] == 8 - 1 - 0.5 and int((l[0] != 8).sum()) == 3


# ---------------- the host packer ----------------
def _rows(seqs, rows=None, pend=None):
    """pack_edits -> per row {id: (c, in the prompt, bias)}, the parameters and pend_src."""
    rows = len(seqs) if rows is None else rows
    img, E = penalties.pack_edits(seqs, rows, pend)
    assert img.dtype == np.int32 and img.shape[0] == LogitEdits.image_words(rows, E)
    ed = LogitEdits.from_image(torch.from_numpy(img), rows, E, torch.zeros(4, dtype=torch.int32))
    rs = ed.row_start.tolist()
    assert rs[0] == 0 and rs[-1] == E and rs == sorted(rs)
    out = []
    for r in range(rows):
        ids = ed.ent_id[rs[r]:rs[r + 1]].tolist()
        assert len(set(ids)) == len(ids)
        w = [x & 0xFFFFFFFF for x in ed.ent_cnt[rs[r]:rs[r + 1]].tolist()]
        b = ed.ent_bias[rs[r]:rs[r + 1]].tolist()
        out.append({t: (x & 0x7FFFFFFF, bool(x >> 31), y) for t, x, y in zip(ids, w, b)})
    return out, ed


def _seq(prompt, out=(), forced=(), **kw):
    s = Sequence(prompt_ids=list(prompt), params=SamplingParams(max_new_tokens=16, **kw), forced_prefix=list(forced))
    s.output_ids += list(out)
    return s


def _oracle(s):
    p = s.params
    return pc.counter_oracle(s.prompt_ids, s.output_ids, p.logit_bias or {}, p.repetition_penalty, PLACEHOLDER)


@pytest.mark.parametrize("rep", [1.0, 1.25], ids=["rep1", "rep1.25"])
def test_packer_matches_the_counter_oracle(rep):
    prompt = [5, 9, 9, 11, 300, 5]
    bias = {9: -3.0, 77: 100.0, 41: 0.5}
    seqs = [_seq(prompt, frequency_penalty=0.5, repetition_penalty=rep),                                  # no outputs
            _seq(prompt, out=[41, 7, 41, 41, 300], presence_penalty=1.0, repetition_penalty=rep),          # repeats
            _seq(prompt, out=[7, 7, PLACEHOLDER], frequency_penalty=0.5, repetition_penalty=rep),          # placeholder
            _seq(prompt, forced=[522, 9], out=[522, 8], frequency_penalty=0.5, repetition_penalty=rep),    # forced prefix
            _seq(prompt, out=[77, 41, 77], logit_bias=bias, repetition_penalty=rep),                       # bias id in the output
            _seq(prompt, out=[1, 2]),                                                                      # not penalised
            _seq(prompt, logit_bias={3: 1.0}, repetition_penalty=rep)]
    got, ed = _rows(seqs, rows=8, pend=[-1, -1, 3, -1, -1, 2, -1])
    for r, s in enumerate(seqs):
        want = _oracle(s) if s.params.penalised else {}
        assert got[r] == want, (r, got[r], want)
    assert got[7] == {} and got[5] == {}
    assert seqs[3].output_ids[:2] == [522, 9] and got[3][522][0] == 2 and got[3][9] == (1, True, 0.0)
    assert got[2][7] == (2, False, 0.0) and PLACEHOLDER not in got[2]
    if rep == 1.0:   # nothing reads the prompt bit: prompt-only ids are left out
        assert set(got[0]) == set() and set(got[1]) == {41, 7, 300} and got[1][300] == (1, True, 0.0)
    else:
        assert set(got[0]) == set(prompt) and got[0][5] == (0, True, 0.0)
    assert got[4][77] == (2, False, 100.0) and got[4][41] == (1, False, 0.5) and got[4][9][2] == -3.0
    # parameters and pending slots; rows without the fields and padding rows are neutral, with no pending token
    assert ed.presence.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and ed.frequency.tolist() == [.5, 0, .5, .5, 0, 0, 0, 0]
    assert ed.repetition.tolist() == [rep] * 5 + [1.0, rep, 1.0]
    assert ed.pend_src.tolist() == [-1, -1, 3, -1, -1, -1, -1, -1]


def test_packer_counts_incrementally_and_across_a_recompute():
    prompt = list(range(100, 140)) + [7]
    s = _seq(prompt, forced=[522], frequency_penalty=1.0, repetition_penalty=1.1, logit_bias={7: 2.0})
    rng = np.random.RandomState(0)
    for step in range(12):
        got, _ = _rows([s])
        assert got[0] == _oracle(s), step
        if step % 3 == 2:            # scheduled ahead: the newest token is a placeholder for one step
            s.output_ids.append(PLACEHOLDER)
            got, _ = _rows([s], pend=[0])
            assert got[0] == _oracle(s)
            s.output_ids[-1] = int(rng.choice([7, 8, 120, 9000]))
        else:
            s.output_ids.append(int(rng.choice([7, 8, 120, 9000])))
        if step == 6:                # recompute preemption: the KV is dropped, the token lists stay
            s.num_computed, s.block_table = 0, []
    fresh = _seq(prompt, forced=[522], out=s.output_ids[1:], frequency_penalty=1.0, repetition_penalty=1.1,
                 logit_bias={7: 2.0})
    assert _rows([s])[0] == _rows([fresh])[0] and s.penalty_state.counted == len(s.output_ids)
    # the prompt's distinct ids: 8192 of them, built once
    big = _seq(list(range(8192)) + [3, 3], out=[3, 9000], repetition_penalty=1.3)
    got, _ = _rows([big])
    assert len(got[0]) == 8193 and got[0][3] == (1, True, 0.0) and got[0][9000] == (1, False, 0.0)
    st = big.penalty_state
    big.output_ids.append(9000)
    assert _rows([big])[0][0][9000] == (2, False, 0.0) and big.penalty_state is st


def test_validation_names_the_field():
    ok = SamplingParams(presence_penalty=-2.0, frequency_penalty=2.0, repetition_penalty=2.0,
                        logit_bias={0: -100.0, 99: 100.0})
    penalties.validate(ok, 100, 1)
    assert ok.penalised and not SamplingParams(logit_bias={}).penalised and not SamplingParams().penalised
    V = 1000   # the vocabulary of every case below
    for field, kw in (("presence_penalty", dict(presence_penalty=2.5)), ("presence_penalty", dict(presence_penalty=-2.01)),
                      ("frequency_penalty", dict(frequency_penalty=-3.0)), ("frequency_penalty", dict(frequency_penalty=float("nan"))),
                      ("repetition_penalty", dict(repetition_penalty=0.0)), ("repetition_penalty", dict(repetition_penalty=2.5)),
                      ("logit_bias", dict(logit_bias={V: 1.0})), ("logit_bias", dict(logit_bias={-1: 1.0})),
                      ("logit_bias", dict(logit_bias={5: 100.5})), ("logit_bias", dict(logit_bias={5: float("nan")})),
                      ("logit_bias", dict(logit_bias={i: 1.0 for i in range(301)}))):
        with pytest.raises(ValueError, match=field):
            penalties.validate(SamplingParams(**kw), V, 1)
    penalties.validate(SamplingParams(logit_bias={V - 1: 1.0}), V, 1)
    penalties.validate(SamplingParams(logit_bias={i: 1.0 for i in range(300)}), 1000, 1)
    with pytest.raises(ValueError, match="TP"):
        penalties.validate(SamplingParams(presence_penalty=0.5), 100, 2)
    penalties.validate(SamplingParams(), 100, 2)   # a neutral request is served under TP as before


# ---------------- engine (tiny-llama) ----------------
@pytest.fixture(scope="module")
def tiny():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=8, graph_buckets=(1, 2, 4, 8),
                                     kv_cache_tokens=8192, max_model_len=512))
    return eng, EngineLLM(eng, max_new_tokens=8)


Q = "list pods in prod"
N = 8
FREE = dict(max_new_tokens=N, ignore_eos=True, safe_decode=False)
# the request of (c): seeded sampling with all four fields
PEN = dict(max_new_tokens=N, ignore_eos=True, temperature=0.9, top_k=50, seed=7, presence_penalty=0.5,
           frequency_penalty=1.2, repetition_penalty=1.3, logit_bias={1000: 4.0, 2000: -100.0})


def _alone(eng, be, query, params, forced=True):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params, forced_prefix=be._forced if forced else None)[0]


def test_bias_plus_100_forces_a_token_and_minus_100_bans_tokens(tiny):
    eng, be = tiny
    tok = eng.tokenizer
    g = _alone(eng, be, Q, SamplingParams(**FREE), forced=False)
    t = next(i for i in range(1000, 2000) if not tok.is_eos(i) and i not in g.output_ids)
    before = eng.runner.stats["penalty_steps"]
    # (a) +100 on an allowed non-EOS token: every generated token is that token, finish `length`
    a = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, safe_decode=False, logit_bias={t: 100.0}), forced=False)
    assert a.output_ids == [t] * N and a.finish_reason == "length"
    assert eng.runner.stats["penalty_steps"] == before + N
    # (b) -100 on every token of the unpenalised greedy completion removes all of them
    b = _alone(eng, be, Q, SamplingParams(**FREE, logit_bias={i: -100.0 for i in g.output_ids}), forced=False)
    assert len(b.output_ids) == N and not set(b.output_ids) & set(g.output_ids)
    # the token mask still wins: +100 on a token no mask row allows changes nothing
    bits = eng.runner.mask_bits.numpy().view(np.uint32)
    banned = next(i for i in range(eng.runner.cfg.vocab_size) if not any((int(row[i // 32]) >> (i % 32)) & 1 for row in bits))
    safe = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True))
    m = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True, logit_bias={banned: 100.0}))
    assert m.output_ids == safe.output_ids and banned not in m.output_ids


def test_frequency_penalty_stops_a_loop(tiny):
    """What the fields are sent for: the greedy completion repeats itself, the penalised one does not."""
    eng, be = tiny
    g = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True))
    assert len(set(g.generated)) < len(g.generated)
    f = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True, frequency_penalty=2.0, presence_penalty=2.0))
    assert len(set(f.generated)) > len(set(g.generated))


def test_same_tokens_through_every_launch_path(tiny):
    """(c): alone and synchronous, chained behind tokens still on the device, in a threaded batch with
    lookahead and mixed company, and across a preemption."""
    eng, be = tiny
    want = _alone(eng, be, Q, SamplingParams(**PEN))
    plain = _alone(eng, be, Q, SamplingParams(**{k: v for k, v in PEN.items() if k in ("max_new_tokens", "ignore_eos",
                                                                                       "temperature", "top_k", "seed")}))
    assert want.output_ids != plain.output_ids and 2000 not in want.output_ids and -1 not in want.output_ids
    # chained / lookahead: the newest token of every decode step is counted on the device
    eng.bm.reset_prefix_cache()
    s = sc.new_sequence(be, Q, SamplingParams(**PEN))
    assert sc.chain_async(eng, s) == want.output_ids
    # the threaded engine, beside greedy, sampled, logprobs and other penalised requests of other lengths
    others = [("get svc -A", SamplingParams(max_new_tokens=3, ignore_eos=True)),
              ("top nodes", SamplingParams(max_new_tokens=6, ignore_eos=True, frequency_penalty=2.0, logprobs=2)),
              ("describe pod web-1", SamplingParams(max_new_tokens=5, ignore_eos=True, temperature=0.7, seed=3)),
              ("get nodes -o wide", SamplingParams(max_new_tokens=7, ignore_eos=True))]
    alone = [_alone(eng, be, q, p) for q, p in others]
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == 5:
            ev.set()

    n0, c0, sch = eng.lookahead_steps, eng.chained_steps, eng.scheduler
    saved = sch.max_batched_tokens, sch.min_chunk
    sch.max_batched_tokens, sch.min_chunk = 40, 4   # chunked prompts: mixed steps with decode rows scheduled ahead
    eng.start()
    try:
        seqs = [eng.submit(be.prompt_ids(q), p, cb, forced_prefix=be._forced)
                for q, p in [others[0], (Q, SamplingParams(**PEN))] + others[1:]]
        assert ev.wait(60)
    finally:
        eng.shutdown()
        sch.max_batched_tokens, sch.min_chunk = saved
    assert eng.lookahead_steps > n0 and eng.healthy
    assert seqs[1].output_ids == want.output_ids
    for got, ref_run in zip([seqs[0]] + seqs[2:], alone):   # and nobody else's tokens moved
        assert got.output_ids == ref_run.output_ids
    assert len(seqs[2].logprobs) == 6
    # the same request alone on the threaded engine: a prefill, then a decode chain
    eng.bm.reset_prefix_cache()
    one = threading.Event()
    eng.start()
    try:
        s2 = eng.submit(be.prompt_ids(Q), SamplingParams(**PEN), lambda q: one.set(), forced_prefix=be._forced)
        assert one.wait(60)
    finally:
        eng.shutdown()
    assert eng.chained_steps > c0 and s2.output_ids == want.output_ids


def test_same_tokens_across_a_preemption(tiny):
    eng, be = tiny
    p = SamplingParams(**PEN)
    want = _alone(eng, be, Q, p)
    eng.bm.reset_prefix_cache()
    sch = eng.scheduler
    saved = (sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps)
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    seqs = [sc.new_sequence(be, Q, p), sc.new_sequence(be, "get nodes -o wide", SamplingParams(max_new_tokens=N, ignore_eos=True))]
    try:
        step = 0
        for s in seqs:
            sch.add(s)
        while any(not s.finished for s in seqs):
            if step == 4:
                victim = seqs[0]
                assert victim in sch.running and victim.num_generated == 4
                sch._preempt(victim)
            batch = sch.schedule()
            eng._apply(batch, eng.runner.execute(batch))
            sch.on_step_done(batch)
            step += 1
    finally:
        sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = saved
    assert seqs[0].output_ids == want.output_ids


def test_logprobs_stay_the_raw_ones(tiny):
    """(d): the top list describes the unadjusted distribution, and the chosen token's logprob is its raw one."""
    eng, be = tiny
    raw = _alone(eng, be, Q, SamplingParams(**FREE, logprobs=20), forced=False)
    t = next(i for i in range(1000, 2000) if i not in raw.logprobs[0].top_ids)
    pen = _alone(eng, be, Q, SamplingParams(**FREE, logprobs=20, logit_bias={t: 100.0}, frequency_penalty=0.5), forced=False)
    assert pen.output_ids == [t] * N and len(pen.logprobs) == N
    # the first token follows the same prompt: the same bits as without penalties
    assert pen.logprobs[0].top_ids == raw.logprobs[0].top_ids
    assert pen.logprobs[0].top_logprobs == raw.logprobs[0].top_logprobs
    for rec in pen.logprobs:
        # from the adjusted logits the chosen token would be the top entry with a logprob of about 0
        assert t not in rec.top_ids and np.isfinite(rec.logprob) and rec.logprob <= rec.top_logprobs[-1] < 0.0
    # a penalised greedy run whose choice stays inside the top list: the record is that entry's raw value
    g = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True, logprobs=20, frequency_penalty=2.0, presence_penalty=2.0))
    hits = 0
    for tok, rec in zip(g.generated, g.logprobs):
        if tok in rec.top_ids:
            hits += 1
            assert rec.logprob == rec.top_logprobs[rec.top_ids.index(tok)]
        else:
            assert rec.logprob <= rec.top_logprobs[-1]
    assert hits > 0 and any(tok != rec.top_ids[0] for tok, rec in zip(g.generated, g.logprobs))


def test_neutral_request_takes_the_greedy_path(tiny):
    """(e)"""
    eng, be = tiny
    st = eng.runner.stats
    before = dict(st)
    staged = []
    orig = eng.runner._stage_samp
    eng.runner._stage_samp = lambda *a, **k: staged.append(orig(*a, **k)) or staged[-1]
    try:
        want = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True))
        got = _alone(eng, be, Q, SamplingParams(max_new_tokens=N, ignore_eos=True, presence_penalty=0.0, frequency_penalty=0.0,
                                                repetition_penalty=1.0, logit_bias={}))
    finally:
        eng.runner._stage_samp = orig
    assert got.output_ids == want.output_ids and got.penalty_state is None
    assert staged and all(x is None for x in staged)   # no sampling arrays: the greedy kernels / graph replays
    assert all(st[k] == before[k] for k in ("penalty_steps", "sampled_steps", "logprob_steps"))


def test_submit_refuses_bad_fields_and_tp(tiny):
    eng, be = tiny
    for field, kw in (("presence_penalty", dict(presence_penalty=3.0)), ("frequency_penalty", dict(frequency_penalty=-2.5)),
                      ("repetition_penalty", dict(repetition_penalty=0.0)),
                      ("logit_bias", dict(logit_bias={eng.runner.cfg.vocab_size: 1.0})),
                      ("logit_bias", dict(logit_bias={5: 101.0})), ("logit_bias", dict(logit_bias={i: 0.5 for i in range(301)}))):
        with pytest.raises(ValueError, match=field):
            eng.submit([1, 2, 3], SamplingParams(**kw), lambda s: None)
    eng.runner.tp_size = 2
    try:
        with pytest.raises(ValueError, match="TP"):
            eng.submit([1, 2, 3], SamplingParams(logit_bias={5: 1.0}), lambda s: None)
    finally:
        eng.runner.tp_size = 1


# ---------------- HTTP ----------------
def _client(be):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.config import Settings
    return TestClient(create_app(Settings(RATE_LIMIT="1000/minute", MODEL="tiny-llama"), backend=be))


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "list pods"}], "max_tokens": 6}
URL = "/v1/chat/completions"


def test_http_fields_change_the_completion(tiny):
    eng, be = tiny
    tok = eng.tokenizer
    # the plain completion's token ids, taken before the API starts the engine's own thread
    eng.bm.reset_prefix_cache()
    g = eng.generate_blocking([be.chat_ids(BODY["messages"])], SamplingParams(max_new_tokens=6, safe_decode=False))[0]
    with _client(be) as c:
        before = eng.runner.stats["penalty_steps"]
        plain = c.post(URL, json=BODY)
        assert plain.status_code == 200 and eng.runner.stats["penalty_steps"] == before
        # the fields sent with their neutral values: the body it always was, and no penalty step
        same = c.post(URL, json=dict(BODY, presence_penalty=0, frequency_penalty=0.0, repetition_penalty=1.0, logit_bias={}))
        assert same.status_code == 200 and eng.runner.stats["penalty_steps"] == before
        pj, sj = plain.json(), same.json()
        assert set(pj) == set(sj) == {"id", "object", "created", "model", "choices", "usage"}
        assert pj["choices"] == sj["choices"] and pj["usage"] == sj["usage"]
        assert set(pj["choices"][0]) == {"index", "message", "finish_reason"}
        # (a) over HTTP, OpenAI's wire form: string keys
        t = next(i for i in range(1000, 2000) if not tok.is_eos(i) and tok.decode([i]).strip())
        r = c.post(URL, json=dict(BODY, logit_bias={str(t): 100}))
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        assert ch["message"]["content"] == tok.decode([t] * 6) and ch["finish_reason"] == "length"
        assert r.json()["usage"]["completion_tokens"] == 6 and eng.runner.stats["penalty_steps"] == before + 6
        # (b) over HTTP: ban the plain completion's tokens
        assert tok.decode([x for x in g.output_ids if not tok.is_eos(x)]) == pj["choices"][0]["message"]["content"]
        r = c.post(URL, json=dict(BODY, logit_bias={str(x): -100 for x in g.output_ids}))
        assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"] != pj["choices"][0]["message"]["content"]
        # the penalties, with logprobs
        r = c.post(URL, json=dict(BODY, frequency_penalty=1.5, presence_penalty=-0.5, repetition_penalty=1.2, logprobs=True,
                                  top_logprobs=2))
        assert r.status_code == 200 and len(r.json()["choices"][0]["logprobs"]["content"]) > 0


def test_http_validation(tiny):
    eng, be = tiny
    with _client(be) as c:
        bad = [dict(presence_penalty=2.1), dict(presence_penalty=-2.1), dict(presence_penalty="x"),
               dict(frequency_penalty=2.5), dict(frequency_penalty=-2.01),
               dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=2.01),
               dict(logit_bias={"abc": 1}), dict(logit_bias={"1.5": 1}), dict(logit_bias={"-3": 1}), dict(logit_bias={"": 1}),
               dict(logit_bias={"5": 100.5}), dict(logit_bias={"5": -101}), dict(logit_bias={"5": "much"}), dict(logit_bias=[5]),
               dict(logit_bias={str(i): 1 for i in range(301)})]
        for kw in bad:
            assert c.post(URL, json=dict(BODY, **kw)).status_code == 422, kw
        good = [dict(presence_penalty=2, frequency_penalty=-2, repetition_penalty=2), dict(repetition_penalty=0.01),
                dict(logit_bias={"5": -100, "7": 100}), dict(logit_bias={str(i): 1 for i in range(300)})]
        for kw in good:
            assert c.post(URL, json=dict(BODY, **kw)).status_code == 200, kw
        # an id past the vocabulary: only the engine knows the vocabulary -> 400
        r = c.post(URL, json=dict(BODY, logit_bias={str(eng.runner.cfg.vocab_size): 1}))
        assert r.status_code == 400 and "logit_bias" in r.text
        assert c.post(URL, json=dict(BODY, logit_bias={str(eng.runner.cfg.vocab_size - 1): 1})).status_code == 200


def test_http_penalties_under_tp_are_refused(tiny):
    eng, be = tiny
    eng.runner.tp_size = 2   # stands in for a tensor-parallel engine: submit refuses before anything runs
    try:
        with _client(be) as c:
            for kw in (dict(frequency_penalty=0.5), dict(presence_penalty=0.5), dict(repetition_penalty=1.1),
                       dict(logit_bias={"5": 1})):
                r = c.post(URL, json=dict(BODY, **kw))
                assert r.status_code == 400 and "TP" in r.text, kw
            assert c.post(URL, json=dict(BODY, frequency_penalty=0)).status_code == 200   # neutral: served as before
    finally:
        eng.runner.tp_size = 1
