"""Guided decoding without a GPU: the regex / choice compiler (engine/guided.py), the mask definition
(ops/reference.py `guide_mask`) against the literal reference of tests/guided_cases.py, the host bookkeeping
(GuideState, GuideTable, pack_guides), the engine on the tiny CPU model and the HTTP fields."""
import itertools
import random
import re
import threading

import numpy as np
import pytest
import torch

from ai_agent_kubectl_amd.engine import guided
from ai_agent_kubectl_amd.engine.sequence import PLACEHOLDER, SamplingParams, Sequence
from tests import engine_helpers
from tests import guided_cases as gc

# (pattern, the 6-character alphabet its strings are drawn from); together they use every construct of the dialect
PATTERNS = [
    (r"abc", "abcd x"),
    (r"a|b|cd", "abcd x"),
    (r"a*b+c?", "abcd x"),
    (r"(ab|cd)*e", "abcde "),
    (r"(?:ab)+c", "abc dx"),
    (r"a{3}", "ab cdx"),
    (r"a{2,}b", "ab cdx"),
    (r"(ab){1,2}c{0,3}", "abc dx"),
    (r"a.c", "abc\n.x"),
    (r".*x", "ax\n b."),
    (r"[abc]+", "abcd x"),
    (r"[a-c]x[^a-c]", "abcdx "),
    (r"[^x]*", "xab\n 1"),
    (r"[a\-c]+", "a-cb x"),
    (r"[]a]+b", "]ab[ x"),
    (r"[\d.]+", "01.a x"),
    (r"\d+\.\d{2}", "019.a "),
    (r"\w+\s\w*", "a_1 \t-"),
    (r"\D\W\S", "a1 -_\n"),
    (r"\S+\s?", "ab \n\t1"),
    (r"a\.\*\\", "ab.*c\\"),
    (r"\(a\)|\[\{\}\]", "()[]a{"),
    (r"\{\}\|\?\+", "{}|?+a"),
    (r"a\nb\tc\r?", "abc\n\t\r"),
    (r"^ab$", "ab^$ x"),
    (r"a\$", "a$b\\ x"),
    (r"(a|b|)c", "abc dx"),
    (r"a||b", "ab| cx"),
    (r"((a|b)(c|d))+", "abcd x"),
    (r"é+a?", "éaeb x"),
    (r"€(x|y)*", "€xyz a"),
    (r"(a*)*b", "ab cdx"),
    (r"x{0}y", "xy abc"),
    (r"kubectl (get|describe) (pods|nodes|svc) -n [a-z0-9-]+", "kgpn -"),
]


# longer strings for the patterns whose matches exceed five characters: matches and near misses
EXTRA = {PATTERNS[-1][0]: ["kubectl get pods -n kp-", "kubectl describe svc -n n", "kubectl get pods -n ", "kubectl get pod -n k",
                           "kubectl get nodes -n K", "kubectl  get pods -n k", "kubectl describe nodes -n -9z"]}


def _accepts(g, data: bytes, table=None) -> bool:
    """A walk of the raw arrays (not Guide.walk)."""
    table = table if table is not None else g.trans.tolist()
    s = 0
    for b in data:
        s = table[s][b]
        if s == 0xFFFF:
            return False
    return bool(g.accept[s])


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=[p for p, _ in PATTERNS])
def test_compiler_agrees_with_re_fullmatch(pattern, alphabet):
    assert len(PATTERNS) >= 25 and len(set(alphabet)) == 6
    g = guided.compile_regex(pattern)
    table = g.trans.tolist()
    rx = re.compile(pattern)
    strings = ["".join(t) for n in range(6) for t in itertools.product(alphabet, repeat=n)]
    rng = random.Random(pattern)
    strings += ["".join(rng.choice(alphabet) for _ in range(rng.randint(6, 14))) for _ in range(200)]
    strings += EXTRA.get(pattern, [])
    hits = 0
    for s in strings:
        want = rx.fullmatch(s) is not None
        hits += want
        assert _accepts(g, s.encode("utf-8"), table) == want, (pattern, s)
    assert hits > 0, "the alphabet never produces a match: the comparison would only test rejections"


@pytest.mark.parametrize("pattern", [p for p, _ in PATTERNS] + ["choice"])
def test_guides_are_trimmed(pattern):
    """A graph check on `trans`: every state is reachable from 0 and reaches an accepting state."""
    g = guided.compile_choice(["pods", "po", "nodes", "svc"]) if pattern == "choice" else guided.compile_regex(pattern)
    S = g.nstates
    assert g.trans.dtype == np.uint16 and g.trans.shape == (S, 256) and g.accept.dtype == np.uint8 and g.accept.shape == (S,)
    succ = [set(int(t) for t in row if t != 0xFFFF) for row in g.trans]
    assert all(t < S for ts in succ for t in ts)
    seen, stack = {0}, [0]
    while stack:
        for t in succ[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    assert seen == set(range(S))
    good = {s for s in range(S) if g.accept[s]}
    grew = True
    while grew:
        more = {s for s in range(S) if s not in good and succ[s] & good}
        grew = bool(more)
        good |= more
    assert good == set(range(S))


REJECTED = [(r"(a)\1", "backreference"), (r"a(?=b)", "lookaround"), (r"a(?!b)", "lookaround"), (r"(?<=a)b", "lookaround"),
            (r"(?<!a)b", "lookaround"), (r"a*?", "lazy"), (r"a+?", "lazy"), (r"a??", "lazy"), (r"a{2}?", "lazy"),
            (r"a*+", "possessive"), (r"a++", "possessive"), (r"a^b", "anchor"), (r"a$b", "anchor"), (r"\bfoo", "anchor"),
            (r"foo\Z", "anchor"), (r"[é]", "non-ASCII"), (r"[a-é]", "non-ASCII"), (r"(?P<n>a)", "group extension"),
            (r"(?i)a", "group extension"), (r"a{2,1}", "n < m"), (r"a{x}", "malformed"), (r"a{", "malformed"),
            (r"(a", "unbalanced"), (r"a)", "unbalanced"), (r"*a", "nothing to repeat"), (r"a|*", "nothing to repeat"),
            (r"[abc", "unterminated"), (r"[z-a]", "bad range"), (r"a\\"[:-1], "trailing backslash"), (r"\x41", "escape"),
            (r"\pL", "escape"), (r"a**", "quantifier after a quantifier"), (r"a+*", "quantifier after a quantifier"),
            (r"a{2}{3}", "quantifier after a quantifier"), (r"(a|b)?*", "quantifier after a quantifier")]


@pytest.mark.parametrize("pattern,names", REJECTED, ids=[p for p, _ in REJECTED])
def test_rejected_constructs_are_named_with_their_offset(pattern, names):
    with pytest.raises(ValueError, match=re.escape(names)) as e:
        guided.compile_regex(pattern)
    assert "offset" in str(e.value)


def test_caps():
    guided.compile_regex("(a|b)" * 409 + "abc")          # 2048 characters
    with pytest.raises(ValueError, match="at most 2048"):
        guided.compile_regex("(a|b)" * 409 + "abcd")
    with pytest.raises(ValueError, match="non-empty"):
        guided.compile_regex("")
    assert guided.compile_regex(r"[a-z]{1,2046}").nstates == 2047
    for p in (r"[a-z]{1,2000}[0-9]{1,2000}", r".{2048}.", r"(a|b)*a(a|b){12}"):
        with pytest.raises(ValueError, match="more than 2048 DFA states"):
            guided.compile_regex(p)
    with pytest.raises(ValueError, match="repeats more than"):
        guided.compile_regex(r"a{4000}")
    with pytest.raises(ValueError, match="NFA states"):
        guided.compile_regex(r"((a{500}){500})")
    guided.compile_choice(["c%d" % i for i in range(256)])
    with pytest.raises(ValueError, match="at most 256"):
        guided.compile_choice(["c%d" % i for i in range(257)])
    with pytest.raises(ValueError, match="non-empty"):
        guided.compile_choice([])
    guided.compile_choice(["x" * 256])
    for bad in (["x" * 257], ["ok", ""], ["é" * 129]):
        with pytest.raises(ValueError, match=r"1\.\.256 bytes"):
            guided.compile_choice(bad)
    with pytest.raises(ValueError, match="more than 2048 DFA states"):
        guided.compile_choice([chr(97 + i) * 250 for i in range(10)])


ADVERSARIAL = [r"((a|b|c|d|e|f)*){0,2000}x", r"(a{0,1000}){0,30}", r"(a?){2000}a{2000}", r"((a|b)*){2000}",
               r"(((a?){40}){40}){2}", r"((a?){50}b?){50}", r"(\w*){1500}", "(" * 1000 + "a" + ")" * 1000,
               "(a?" * 500 + ")" * 500 + "{2,}"]


@pytest.mark.parametrize("pattern", ADVERSARIAL, ids=[p[:24] for p in ADVERSARIAL])
def test_short_expensive_patterns_are_refused_quickly(pattern):
    """The caps bound the compiler's work, not only its result: nested counted repetition is refused in a
    fraction of a second instead of occupying the server (the bound is generous: 10-100 ms are typical)."""
    import time
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="NFA states|units of work|DFA states|nests groups too deeply"):
        guided.compile_regex(pattern)
    assert time.perf_counter() - t0 < 1.0


def test_large_legitimate_patterns_fit_the_work_budget():
    import time
    t0 = time.perf_counter()
    assert guided.compile_regex(r"[a-z]{1,2046}").nstates == 2047
    assert guided.compile_regex(r"a{2047}").nstates == 2048
    assert guided.compile_regex(r"(\w+ ){1,50}\w+").nstates > 50
    assert guided.compile_regex("|".join("word%d" % i for i in range(250))).nstates > 20
    assert time.perf_counter() - t0 < 2.0


def test_compile_choice_accepts_exactly_the_choices():
    choices = ["pods", "po", "nodes", "services", "svc", "naïve", "a b"]
    g = guided.compile_choice(choices)
    for c in choices:
        assert _accepts(g, c.encode("utf-8"))
    others = {c[:n] for c in choices for n in range(len(c))} | {c + "x" for c in choices} | {"", "x", "Pods"}
    for s in others - set(choices):
        assert not _accepts(g, s.encode("utf-8")), s
    assert g.key == guided.compile_choice(list(choices)).key != guided.compile_choice(choices[:-1]).key
    assert guided.compile_regex("ab").key == guided.compile_regex("ab").key != guided.compile_regex("ab?").key


# ---------------- the mask ----------------
def test_case_preconditions():
    gc.check_preconditions()


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.id)
def test_reference_mask_is_the_literal_definition(case):
    bits, idx, after = gc.literal(case)
    got = gc.run_ops(case, "cpu")
    assert got[0].dtype == torch.int32 and got[0].shape == bits.shape
    assert np.array_equal(got[0].numpy().view(np.uint32), bits)
    assert np.array_equal(got[1].numpy(), idx) and np.array_equal(got[2].numpy(), after)


# ---------------- host bookkeeping ----------------
class _Tok:
    eos_ids = (2,)
    id_to_bytes = [b"a", b"bc", None, b"d", b"abc", b"x"]
    vocab_size = 6

    def is_eos(self, t):
        return t in self.eos_ids

    def token_bytes(self, t):
        return self.id_to_bytes[t] or b""

    def decode(self, ids):
        return b"".join(self.token_bytes(t) for t in ids).decode()


def test_guide_state_across_placeholders_and_a_recompute():
    g = guided.compile_regex(r"a(bc)+d?")
    tok = _Tok()
    s = Sequence(prompt_ids=[5, 5], params=SamplingParams(guide=g), forced_prefix=[0])   # the prefix spells "a"
    st = guided.state_of(s, tok)
    assert st.counted == 1 and st.state == g.walk(0, b"a")
    s.output_ids.append(PLACEHOLDER)             # a step in flight: not walked
    assert guided.state_of(s, tok).counted == 1 and st.state == g.walk(0, b"a")
    s.output_ids[-1] = 1                          # settled: "bc"
    s.output_ids.append(PLACEHOLDER)
    assert guided.state_of(s, tok).counted == 2 and st.state == g.walk(0, b"abc")
    s.output_ids[-1] = 2                          # EOS does not move the state
    assert guided.state_of(s, tok).counted == 3 and st.state == g.walk(0, b"abc")
    # a recompute preemption drops the KV, not the outputs: the state stays valid and nothing is walked twice
    s.num_computed, s.block_table = 0, []
    s.output_ids.append(1)
    assert guided.state_of(s, tok) is st and st.counted == 4 and st.state == g.walk(0, b"abcbc")
    s.output_ids.append(5)                        # "x": dead, and it stays dead
    s.output_ids.append(1)
    assert guided.state_of(s, tok).state == -1
    s2 = Sequence(prompt_ids=[5], params=SamplingParams(guide=g))
    s2.output_ids += [0, 2 + 0]                   # a token without bytes that is not EOS would kill; id 2 is EOS here
    assert guided.state_of(s2, tok).state == g.walk(0, b"a")


def test_guide_table_placement_sharing_reuse_and_full():
    a, b, c = guided.compile_regex("a{9}"), guided.compile_regex("b{5}"), guided.compile_regex("c{3}")
    assert (a.nstates, b.nstates, c.nstates) == (10, 6, 4)
    t = guided.GuideTable(states=16, device="cpu")
    pa, pb = t.acquire(a), t.acquire(b)
    assert (pa.base, pb.base) == (0, 10) and t.acquire(guided.compile_regex("a{9}")) is pa and pa.refs == 2
    t.flush()
    assert t.uploads == 2
    assert np.array_equal(t.trans[10:16].numpy().view(np.uint16), b.trans) and np.array_equal(t.accept[:10].numpy(), a.accept)
    with pytest.raises(ValueError, match="guide table is full"):
        t.acquire(c)                               # 16 states, all held by live sequences
    t.release(pb)
    assert t.acquire(b) is pb and t.uploads == 2   # idle guides stay resident: no second upload
    t.release(pb)
    pc = t.acquire(c)                              # ... until their range is needed
    assert pc.base == 10 and b.key not in t.placed
    t.flush()
    assert t.uploads == 3 and np.array_equal(t.trans[10:14].numpy().view(np.uint16), c.trans)
    assert np.array_equal(t.trans[:10].numpy().view(np.uint16), a.trans)   # the neighbour is untouched
    t.release(pa), t.release(pa), t.release(pc)
    with pytest.raises(ValueError, match="guide table is full"):
        t.acquire(guided.compile_regex("d{16}"))   # 17 states never fit
    big = t.acquire(guided.compile_regex("d{15}"))  # evicts both idle guides
    assert big.base == 0 and len(t.placed) == 1


def test_pack_guides_layout():
    g = guided.compile_regex(r"a(bc)+d?")
    tok = _Tok()
    t = guided.GuideTable(states=32, device="cpu")
    t.acquire(guided.compile_regex("zz"))
    seqs = [Sequence(prompt_ids=[5], params=SamplingParams()), Sequence(prompt_ids=[5], params=SamplingParams(guide=g)),
            Sequence(prompt_ids=[5], params=SamplingParams(guide=g))]
    seqs[1].guide_ref = seqs[2].guide_ref = t.acquire(g)
    seqs[2].output_ids += [0, PLACEHOLDER]
    img = guided.pack_guides(seqs, 4, [-1, -1, 2], tok)
    assert img.dtype == np.int32 and img.shape == (16,)
    base = seqs[1].guide_ref.base
    assert base == 3
    assert img[0:4].tolist() == [-1, base, base, -1]                 # arena bases; padding and plain rows -1
    assert img[4:8].tolist() == [0, g.nstates, g.nstates, 0]
    assert img[8:12].tolist() == [0, 0, g.walk(0, b"a"), 0]
    assert img[12:16].tolist() == [-1, -1, 2, -1]
    assert guided.pack_guides(seqs, 3, None, tok)[9:].tolist() == [-1, -1, -1]


def test_validate():
    tok = _Tok()
    guided.validate(SamplingParams(), tok, 8)                        # not guided: nothing to check, also under TP
    g = guided.compile_regex(r"a(bc)+d?")
    with pytest.raises(ValueError, match="TP"):
        guided.validate(SamplingParams(guide=g), tok, 2)
    with pytest.raises(ValueError, match="this tokenizer cannot spell the pattern"):
        guided.validate(SamplingParams(guide=g), tok, 1)             # no single-byte token spells "b"
    ok = guided.compile_regex(r"a+d?")
    guided.validate(SamplingParams(guide=ok), tok, 1)
    guided.validate(SamplingParams(guide=ok), tok, 1, forced_prefix=[0, 0])
    with pytest.raises(ValueError, match="forced prefix"):
        guided.validate(SamplingParams(guide=ok), tok, 1, forced_prefix=[3])


# ---------------- engine (tiny-llama) ----------------
@pytest.fixture(scope="module")
def tiny():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=8, graph_buckets=(1, 2, 4, 8),
                                     kv_cache_tokens=8192, max_model_len=512))
    return eng, EngineLLM(eng, max_new_tokens=8)


Q = "list pods in prod"
PAT = r"kubectl (get|describe) (pods|nodes|svc) -n [a-z0-9-]{1,6}"
CHOICES = ["pods", "nodes", "services", "deployments"]


def _text(eng, seq):
    tok = eng.tokenizer
    return tok.decode([t for t in seq.output_ids if not tok.is_eos(t)])


def _alone(eng, be, query, params, forced=False):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params, forced_prefix=be._forced if forced else None)[0]


def test_guided_choice_returns_one_of_the_choices(tiny):
    eng, be = tiny
    before = eng.runner.stats["guided_steps"]
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=32, safe_decode=False, guide=guided.compile_choice(CHOICES)))
    assert _text(eng, s) in CHOICES and s.finish_reason == "stop"
    assert eng.runner.stats["guided_steps"] == before + len(s.output_ids)
    assert s.guide_ref is None and all(p.refs == 0 for p in eng.runner.guide_table.placed.values())


def test_guided_regex_matches_or_is_a_prefix(tiny):
    eng, be = tiny
    g = guided.compile_regex(PAT)
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=False, guide=g))
    assert s.finish_reason == "stop" and re.fullmatch(PAT, _text(eng, s)), _text(eng, s)
    short = _alone(eng, be, Q, SamplingParams(max_new_tokens=3, safe_decode=False, guide=g))
    text = _text(eng, short)
    assert short.finish_reason == "length" and len(short.output_ids) == 3 and s.output_ids[:3] == short.output_ids
    assert g.is_prefix(text.encode()) and not re.fullmatch(PAT, text) and _text(eng, s).startswith(text)
    # seeded sampling: still a match, and the same bytes again
    p = SamplingParams(max_new_tokens=48, safe_decode=False, guide=g, temperature=1.0, seed=5)
    a, b = _alone(eng, be, Q, p), _alone(eng, be, Q, p)
    assert a.finish_reason == "stop" and re.fullmatch(PAT, _text(eng, a)) and a.output_ids == b.output_ids
    other = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=False, guide=g, temperature=1.0, seed=6))
    assert re.fullmatch(PAT, _text(eng, other)) and other.output_ids != a.output_ids != s.output_ids


def test_safe_decode_and_a_guide_through_the_forced_prefix(tiny):
    eng, be = tiny
    g = guided.compile_regex(PAT)
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=True, guide=g), forced=True)
    assert s.output_ids[:len(be._forced)] == be._forced and s.finish_reason == "stop"
    assert re.fullmatch(PAT, _text(eng, s)), _text(eng, s)
    done = []
    with pytest.raises(ValueError, match="forced prefix"):   # the reply starts with "kubectl": this guide cannot follow
        eng.submit(be.prompt_ids(Q), SamplingParams(guide=guided.compile_choice(CHOICES)), done.append, forced_prefix=be._forced)


def test_logprobs_of_a_guided_request_stay_inside_the_guide(tiny):
    eng, be = tiny
    g = guided.compile_regex(PAT)
    tok = eng.tokenizer
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=False, guide=g, logprobs=20))
    assert len(s.logprobs) == len(s.generated) and re.fullmatch(PAT, _text(eng, s))
    state, short_lists = 0, 0
    for t, rec in zip(s.generated, s.logprobs):
        live = [i for i in rec.top_ids if i >= 0]
        short_lists += len(live) < 20
        for i, lp in zip(rec.top_ids, rec.top_logprobs):
            if i < 0:
                assert lp == float("-inf")          # fewer than 20 tokens are allowed here
            elif tok.is_eos(i):
                assert g.accept[state]
            else:
                assert tok.token_bytes(i) and g.walk(state, tok.token_bytes(i)) >= 0, (state, tok.token_bytes(i))
        assert t in live and np.isfinite(rec.logprob) and rec.logprob <= 0.0
        assert abs(sum(np.exp(rec.top_logprobs[:len(live)])) - 1.0) < 1e-3 or len(live) == 20
        state = state if tok.is_eos(t) else g.walk(state, tok.token_bytes(t))
    assert short_lists > 0


OTHERS = [("get svc -A", dict(max_new_tokens=3, ignore_eos=True)),
          ("top nodes", dict(max_new_tokens=6, ignore_eos=True, frequency_penalty=2.0, logprobs=2)),
          ("describe pod web-1", dict(max_new_tokens=5, ignore_eos=True, temperature=0.7, seed=3)),
          ("get nodes -o wide", dict(max_new_tokens=7, ignore_eos=True))]


@pytest.mark.parametrize("lookahead", [True, False], ids=["lookahead", "no-lookahead"])
def test_same_bytes_alone_and_in_mixed_company(tiny, lookahead):
    eng, be = tiny
    g = guided.compile_regex(PAT)
    pg = dict(max_new_tokens=48, safe_decode=False, guide=g)
    ps = dict(pg, temperature=0.9, seed=11)
    want_g, want_s = _alone(eng, be, Q, SamplingParams(**pg)), _alone(eng, be, Q, SamplingParams(**ps))
    alone = [_alone(eng, be, q, SamplingParams(**kw), forced=True) for q, kw in OTHERS]
    # chained behind a token still on the device
    eng.bm.reset_prefix_cache()
    assert gc.chain_async(eng, Sequence(prompt_ids=be.prompt_ids(Q), params=SamplingParams(**ps))) == want_s.output_ids
    # one prompt admitted per step: every step after the first is a mixed decode + prefill step
    eng.bm.reset_prefix_cache()
    outs = engine_helpers.run_staggered(eng, [be.prompt_ids(Q), be.prompt_ids(Q)], SamplingParams(**pg), [])
    assert outs == [want_g.output_ids] * 2 and engine_helpers.run_staggered.mixed > 0
    # the threaded engine beside greedy, sampled, penalised and logprobs requests of other lengths
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == len(OTHERS) + 2:
            ev.set()

    n0, sch = eng.lookahead_steps, eng.scheduler
    saved = sch.max_batched_tokens, sch.min_chunk, eng.lookahead
    sch.max_batched_tokens, sch.min_chunk, eng.lookahead = 40, 4, lookahead
    g0 = eng.runner.stats["guided_steps"]
    eng.start()
    try:
        first = eng.submit(be.prompt_ids(OTHERS[0][0]), SamplingParams(**OTHERS[0][1]), cb, forced_prefix=be._forced)
        a = eng.submit(be.prompt_ids(Q), SamplingParams(**pg), cb)
        b = eng.submit(be.prompt_ids(Q), SamplingParams(**ps), cb)
        rest = [eng.submit(be.prompt_ids(q), SamplingParams(**kw), cb, forced_prefix=be._forced) for q, kw in OTHERS[1:]]
        assert ev.wait(120)
    finally:
        eng.shutdown()
        sch.max_batched_tokens, sch.min_chunk, eng.lookahead = saved
    assert eng.healthy and (eng.lookahead_steps > n0) == lookahead
    assert a.output_ids == want_g.output_ids and b.output_ids == want_s.output_ids
    for got, ref_run in zip([first] + rest, alone):   # and nobody else's bytes moved
        assert got.output_ids == ref_run.output_ids
    assert eng.runner.stats["guided_steps"] > g0
    assert all(p.refs == 0 for p in eng.runner.guide_table.placed.values())


def test_plain_requests_stage_nothing_for_guides(tiny):
    eng, be = tiny
    before = eng.runner.stats["guided_steps"]
    staged = []
    orig = eng.runner._stage_guides
    eng.runner._stage_guides = lambda *a, **k: staged.append(1) or orig(*a, **k)
    try:
        _alone(eng, be, Q, SamplingParams(max_new_tokens=4, ignore_eos=True), forced=True)
        _alone(eng, be, Q, SamplingParams(max_new_tokens=4, ignore_eos=True, temperature=0.8, seed=1), forced=True)
    finally:
        eng.runner._stage_guides = orig
    assert not staged and eng.runner.stats["guided_steps"] == before


def test_concurrent_requests_compile_a_source_once(tiny, monkeypatch):
    eng, be = tiny
    calls, gate = [], threading.Event()
    real = guided.compile_regex

    def slow(pattern):
        calls.append(pattern)
        gate.wait(10)
        return real(pattern)

    monkeypatch.setattr(guided, "compile_regex", slow)
    out = []
    ts = [threading.Thread(target=lambda: out.append(be.compile_guide(guided_regex="once[0-9]+"))) for _ in range(4)]
    for t in ts:
        t.start()
    while not calls:
        pass
    gate.set()
    for t in ts:
        t.join(10)
    assert calls == ["once[0-9]+"] and len(out) == 4 and all(g is out[0] for g in out)
    assert not be._compiling and be.compile_guide(guided_regex="once[0-9]+") is out[0]
    # a failed compilation reaches every waiter and leaves nothing behind
    with pytest.raises(ValueError, match="lookaround"):
        be.compile_guide(guided_regex="a(?=b)")
    assert not be._compiling


def test_a_finished_sequence_in_the_inbox_releases_its_guide(tiny):
    eng, be = tiny
    g = guided.compile_regex(r"[a-z]{1,30}")
    s = eng.submit(be.prompt_ids(Q), SamplingParams(max_new_tokens=4, safe_decode=False, guide=g), lambda q: None)
    ref = s.guide_ref
    from ai_agent_kubectl_amd.engine.sequence import SeqStatus
    s.status = SeqStatus.ABORTED          # finished before the engine saw the add
    eng._drain_inbox()
    assert s.guide_ref is None and ref.refs == 0 and s not in eng.scheduler.waiting


def test_abort_releases_the_guide(tiny):
    eng, be = tiny
    g = guided.compile_regex(r"[a-z]{1,40}")
    s = eng.submit(be.prompt_ids(Q), SamplingParams(max_new_tokens=40, safe_decode=False, guide=g), lambda q: None)
    ref = s.guide_ref
    assert ref is not None and ref.refs == 1 and eng.runner.guide_table.placed[g.key] is ref
    eng.abort(s)
    eng._drain_inbox()
    assert s.guide_ref is None and ref.refs == 0


# ---------------- HTTP ----------------
def _client(be):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.config import Settings
    return TestClient(create_app(Settings(RATE_LIMIT="1000/minute", MODEL="tiny-llama"), backend=be))


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "list pods"}], "max_tokens": 40}
URL = "/v1/chat/completions"


def test_http_fields(tiny):
    eng, be = tiny
    with _client(be) as c:
        before, cached = eng.runner.stats["guided_steps"], len(be._guides)
        plain = c.post(URL, json=BODY)
        assert plain.status_code == 200 and eng.runner.stats["guided_steps"] == before
        r = c.post(URL, json=dict(BODY, guided_choice=CHOICES))
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        assert ch["message"]["content"] in CHOICES and ch["finish_reason"] == "stop"
        assert eng.runner.stats["guided_steps"] > before
        # the response keeps its shape
        assert set(r.json()) == set(plain.json()) == {"id", "object", "created", "model", "choices", "usage"}
        assert set(ch) == set(plain.json()["choices"][0]) == {"index", "message", "finish_reason"}
        r = c.post(URL, json=dict(BODY, guided_regex=PAT, temperature=0.8, seed=4, logprobs=True, top_logprobs=3,
                                  frequency_penalty=0.5, logit_bias={"1000": 5}))
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        assert re.fullmatch(PAT, ch["message"]["content"]) and ch["finish_reason"] == "stop"
        assert "".join(e["token"] for e in ch["logprobs"]["content"]) == ch["message"]["content"]
        again = c.post(URL, json=dict(BODY, guided_regex=PAT, temperature=0.8, seed=4, frequency_penalty=0.5,
                                      logit_bias={"1000": 5}))
        assert again.json()["choices"][0]["message"]["content"] == ch["message"]["content"]
        cut = c.post(URL, json=dict(BODY, guided_regex=PAT, max_tokens=2)).json()["choices"][0]
        assert cut["finish_reason"] == "length" and guided.compile_regex(PAT).is_prefix(cut["message"]["content"].encode())
        assert len(be._guides) == cached + 2   # compiled once per source


def test_http_validation(tiny):
    eng, be = tiny
    with _client(be) as c:
        bad = [dict(guided_regex="a+", guided_choice=["a"]), dict(guided_regex=""), dict(guided_choice=[]),
               dict(guided_regex="a" * 2049), dict(guided_choice=["c%d" % i for i in range(257)]),
               dict(guided_choice=["ok", ""]), dict(guided_choice=["x" * 257]), dict(guided_choice="pods"),
               dict(guided_regex=5), dict(guided_choice=[1, 2])]
        for kw in bad:
            assert c.post(URL, json=dict(BODY, **kw)).status_code == 422, kw
        for kw, names in ((dict(guided_regex=r"(a)\1"), "backreference"), (dict(guided_regex=r"a(?=b)"), "lookaround"),
                          (dict(guided_regex=r"a*?"), "lazy"), (dict(guided_regex=r"[a-z]{1,2000}[0-9]{1,2000}"), "DFA states")):
            r = c.post(URL, json=dict(BODY, **kw))
            assert r.status_code == 400 and names in r.text, (kw, r.text)
        good = [dict(guided_regex="(a|b)" * 409 + "abc", max_tokens=2), dict(guided_choice=["x" * 256], max_tokens=2),
                dict(guided_choice=["c%d" % i for i in range(256)])]
        for kw in good:
            assert c.post(URL, json=dict(BODY, **kw)).status_code == 200, kw
        # a tokenizer without the single-byte tokens the pattern needs
        have = guided.single_byte_tokens(eng.tokenizer)
        eng.tokenizer._guided_single_bytes = np.zeros(256, dtype=bool)
        try:
            r = c.post(URL, json=dict(BODY, guided_regex="ab"))
            assert r.status_code == 400 and "cannot spell the pattern" in r.text
        finally:
            eng.tokenizer._guided_single_bytes = have
        # a guide table with no room
        table = eng.runner.guides()
        eng.runner.guide_table = guided.GuideTable(states=4, device="cpu")
        try:
            r = c.post(URL, json=dict(BODY, guided_regex="abcdef"))
            assert r.status_code == 400 and "guide table is full" in r.text
            assert c.post(URL, json=dict(BODY, guided_regex="abc")).status_code == 200
        finally:
            eng.runner.guide_table = table
        # a tensor-parallel engine refuses before anything runs; a request without the fields is served as before
        eng.runner.tp_size = 2
        try:
            for kw in (dict(guided_regex="a+"), dict(guided_choice=["a"])):
                r = c.post(URL, json=dict(BODY, **kw))
                assert r.status_code == 400 and "TP" in r.text, kw
            assert c.post(URL, json=BODY).status_code == 200
        finally:
            eng.runner.tp_size = 1
