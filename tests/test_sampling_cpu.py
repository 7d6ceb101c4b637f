"""Seeded temperature / top-k / top-p sampling on the CPU: the noise function, the reference sampler's
distribution and cuts, the engine's seed contract (the same tokens alone, in mixed company and after a
preemption) and the /v1/chat/completions fields.  The HIP kernel is in test_sampling_gpu.py."""
import math

import numpy as np
import pytest
import torch

from ai_agent_kubectl_amd import ops
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence
from ai_agent_kubectl_amd.ops import reference as ref

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _u_python(seed, position, gid):
    """The issue's noise function in plain Python integers."""
    key = _mix((seed + (position + 1) * GOLD) & M64)
    z = _mix((key + (gid + 1) * GOLD) & M64)
    return (2 * (z >> 41) + 1) * 2.0 ** -24


def _arrays(n, temperature=1.0, top_k=0, top_p=1.0, seed=0, position=None):
    pos = torch.arange(n, dtype=torch.int32) if position is None else torch.full((n,), position, dtype=torch.int32)
    return (torch.full((n,), temperature, dtype=torch.float32), torch.full((n,), top_k, dtype=torch.int32),
            torch.full((n,), top_p, dtype=torch.float32), torch.full((n,), seed, dtype=torch.int64), pos)


# ---------------- noise ----------------
PINS = [((0, 0, 0), 0.6524484753608704), ((7, 3, 128255), 0.5726361870765686),
        ((0xDEADBEEFCAFEF00D, 4095, 12345), 0.2928674817085266)]


@pytest.mark.parametrize("triple,u", PINS)
def test_noise_pins(triple, u):
    got = float(ref.sample_noise_u(triple[0], triple[1], [triple[2]])[0])
    assert got == u == _u_python(*triple)
    assert float(np.float32(got)) == got   # exact in fp32


def test_noise_strictly_inside_unit_interval():
    gids = np.arange(128256)
    for seed, pos in ((0, 0), (M64, 2 ** 31 - 2), (12345, 17)):
        u = ref.sample_noise_u(seed, pos, gids)
        assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
        assert u[5] == _u_python(seed, pos, 5)
        assert len(np.unique(u)) > 120000   # 2^23 values: few collisions
    # the extremes of the formula themselves
    assert (2 * 0 + 1) * 2.0 ** -24 > 0.0 and (2 * (2 ** 23 - 1) + 1) * 2.0 ** -24 < 1.0


# ---------------- distribution ----------------
V, N = 64, 4096
_g = torch.Generator().manual_seed(0)
LOGITS = torch.randn(V, generator=_g).to(torch.bfloat16)


def _chi2_q999(df):
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.999, df))
    except ImportError:   # Wilson-Hilferty
        z = 3.0902323061678132
        return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


def _draws(T, seed, top_k=0, top_p=1.0):
    L = LOGITS[None].expand(N, V).contiguous()
    idx, _ = ref.sample(L, None, None, *_arrays(N, T, top_k, top_p, seed))
    return idx.long()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_token_counts_follow_softmax(T, seed):
    """Positions 0..4095 of one seed are 4096 draws from softmax(l / T): chi-square at the 0.999
    quantile, bins with an expected count below 5 pooled into one."""
    cnt = torch.bincount(_draws(T, seed), minlength=V).double()
    e = torch.softmax(LOGITS.double() / T, 0) * N
    small = e < 5
    stat = float((((cnt - e) ** 2 / e)[~small]).sum())
    df = int((~small).sum()) - 1
    if small.any():
        stat += float((cnt[small].sum() - e[small].sum()) ** 2 / e[small].sum())
        df += 1
    assert df >= 8
    assert stat < _chi2_q999(df), (stat, df)


def test_top_k_draws_only_the_k_largest():
    top5 = set(torch.topk(LOGITS.float(), 5).indices.tolist())
    assert len(set(torch.topk(LOGITS.float(), 6).values.tolist())) == 6   # no tie at the cut: exactly five kept
    drawn = set(_draws(1.0, 1, top_k=5).tolist())
    assert drawn <= top5 and len(drawn) == 5


def test_top_p_draws_only_the_nucleus():
    p = torch.softmax(LOGITS.double(), 0)
    order = torch.argsort(p, descending=True)
    csum = torch.cumsum(p[order], 0)
    n = int((csum >= 0.5).nonzero()[0]) + 1
    nucleus = set(order[:n].tolist())
    drawn = set(_draws(1.0, 2, top_p=0.5).tolist())
    assert drawn <= nucleus and len(drawn) == n
    L = LOGITS[None].contiguous()
    _, _, cut, kept = ref.sample(L, None, None, *_arrays(1, 1.0, 0, 0.5, 2), return_cut=True)
    assert int(kept[0]) == n and float(cut[0]) == float(LOGITS[order[n - 1]])


def test_cuts_keep_ties_and_clamp_k():
    l = torch.tensor([[1.0, 3.0, 2.0, 3.0, 2.0, 2.0, -1.0, 0.5]], dtype=torch.bfloat16)
    for k, want_cut, want_kept in ((1, 3.0, 2), (2, 3.0, 2), (3, 2.0, 5), (8, -1.0, 8), (100, -1.0, 8)):
        _, _, cut, kept = ref.sample(l, None, None, *_arrays(1, 1.0, k, 1.0, 5), return_cut=True)
        assert (float(cut[0]), int(kept[0])) == (want_cut, want_kept), k
    # top-p after top-k: masses e^0 x2, e^-1 x3 -> the value 3 holds 2 / (2 + 3/e) = 0.644 of the kept mass
    _, _, cut, kept, gap, p_lo, p_hi = ref.sample(l, None, None, *_arrays(1, 1.0, 3, 0.6, 5), return_cut=True,
                                                  dtype=torch.float64, return_margins=True)
    assert (float(cut[0]), int(kept[0])) == (3.0, 2)
    share = 2 / (2 + 3 / math.e)
    assert abs(float(p_hi[0]) - (share - 0.6)) < 1e-6 and abs(float(p_lo[0]) - 0.6) < 1e-6   # fp32 0.6
    _, _, cut, kept = ref.sample(l, None, None, *_arrays(1, 1.0, 3, 0.7, 5), return_cut=True)
    assert (float(cut[0]), int(kept[0])) == (2.0, 5)
    # no cut: -inf and every allowed token
    _, _, cut, kept = ref.sample(l, None, None, *_arrays(1, 1.0, 0, 1.0, 5), return_cut=True)
    assert float(cut[0]) == float("-inf") and int(kept[0]) == 8


# ---------------- temperature 0 ----------------
def _mask_bits(words, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 2 ** 32, size=(2, words), dtype=np.uint64)
                            .astype(np.uint32).view(np.int32))


@pytest.mark.parametrize("off", [0, 64])
def test_temperature_zero_is_masked_argmax(off):
    Vv, B = 520, 9
    torch.manual_seed(3)
    logits = torch.randn(B, Vv).to(torch.bfloat16)
    logits[0, :] = 0.0                                   # all equal: the lowest allowed id
    logits[1, [7, 300, 519]] = 9.0                       # tied maxima
    logits[2, [8, 9]] = 9.0
    bits = _mask_bits((Vv + off + 31) // 32)
    midx = torch.tensor([0, 1, -1, 0, 1, -1, 0, 0, 1], dtype=torch.int32)
    t, k, p, s, pos = _arrays(B, 0.0, 3, 0.4, 99)
    for mb, mi in ((None, None), (bits, midx)):
        i0, v0 = ref.masked_argmax(logits, mb, mi, off)
        i1, v1 = ops.sample(logits, mb, mi, t, k, p, s, pos, vocab_offset=off)
        assert torch.equal(i0, i1) and torch.equal(v0, v1)
        # such rows inside a batch whose other rows sample
        t2 = t.clone()
        t2[1::2] = 0.9
        i2, v2 = ops.sample(logits, mb, mi, t2, k, p, s, pos, vocab_offset=off)
        assert torch.equal(i0[0::2], i2[0::2]) and torch.equal(v0[0::2], v2[0::2])
    assert int(ref.masked_argmax(logits, None, None, off)[0][1]) == 7 + off


def test_sample_respects_the_mask_and_the_global_id():
    Vv, off = 256, 64
    logits = torch.zeros(4, Vv, dtype=torch.bfloat16)
    bits = _mask_bits((Vv + off + 31) // 32, seed=1)
    midx = torch.tensor([0, 1, 0, -1], dtype=torch.int32)
    idx, _ = ops.sample(logits, bits, midx, *_arrays(4, 1.0, 0, 1.0, 11, position=0), vocab_offset=off)
    for r in range(3):
        g = int(idx[r])
        assert off <= g < off + Vv
        assert (int(bits[int(midx[r]), g // 32]) >> (g % 32)) & 1
    # equal logits: the token is the argmax of the noise, which is indexed by the global id
    u = ref.sample_noise_u(11, 0, np.arange(off, off + Vv))
    assert int(idx[3]) == off + int(np.argmax(u))


# ---------------- engine (tiny-llama) ----------------
@pytest.fixture(scope="module")
def tiny():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=8, graph_buckets=(1, 2, 4, 8),
                                     kv_cache_tokens=8192, max_model_len=512))
    return eng, EngineLLM(eng, max_new_tokens=8)


SAMPLED = dict(max_new_tokens=8, ignore_eos=True, temperature=0.9, top_k=50, top_p=0.95)


def _alone(eng, be, query, params):
    return eng.generate_blocking([be.prompt_ids(query)], params, forced_prefix=be._forced)[0].output_ids


def _staggered(eng, be, items, preempt=None):
    """One (query, params) admitted per step, like tests/engine_helpers.run_staggered but with each
    request's own params.  preempt = (row, step): that sequence is preempted before the given step."""
    sch = eng.scheduler
    saved = (sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps)
    sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = 0.0, 0.0, 0
    seqs, pending, step = [], list(items), 0
    try:
        while pending or any(not s.finished for s in seqs):
            if pending:
                q, params = pending.pop(0)
                seqs.append(Sequence(prompt_ids=be.prompt_ids(q), params=params, forced_prefix=list(be._forced)))
                sch.add(seqs[-1])
            if preempt is not None and step == preempt[1]:
                victim = seqs[preempt[0]]
                assert victim in sch.running and 0 < victim.num_generated < victim.params.max_new_tokens
                sch._preempt(victim)
            batch = sch.schedule()
            eng._apply(batch, eng.runner.execute(batch))
            sch.on_step_done(batch)
            step += 1
    finally:
        sch.prefill_max_wait_s, sch.gather_max_s, sch.hold_steps = saved
    return [s.output_ids for s in seqs]


def test_engine_seed_gives_the_same_tokens_in_any_company(tiny):
    from tests.engine_helpers import run_staggered
    eng, be = tiny
    p7 = SamplingParams(seed=7, **SAMPLED)
    greedy = SamplingParams(max_new_tokens=8, ignore_eos=True)
    want = _alone(eng, be, "list pods in prod", p7)
    assert _alone(eng, be, "list pods in prod", p7) == want
    assert want != _alone(eng, be, "list pods in prod", greedy)
    before = eng.runner.stats["sampled_steps"]
    # among sampling requests (same params object: run_staggered takes one)
    qs = ["get nodes -o wide", "list pods in prod", "describe svc api", "top pods"]
    eng.bm.reset_prefix_cache()
    outs = run_staggered(eng, [be.prompt_ids(q) for q in qs], p7, be._forced)
    assert run_staggered.mixed >= 3 and outs[1] == want
    # among greedy and differently seeded requests
    eng.bm.reset_prefix_cache()
    items = [("get nodes -o wide", greedy), ("describe svc api", SamplingParams(seed=8, **SAMPLED)),
             ("list pods in prod", p7), ("top pods", greedy), ("scale web to 3", SamplingParams(**SAMPLED))]
    outs = _staggered(eng, be, items)
    assert outs[2] == want
    assert outs[0] == _alone(eng, be, "get nodes -o wide", greedy)   # greedy rows of a sampled step stay greedy
    assert eng.runner.stats["sampled_steps"] > before
    assert all(eng.bm.ref_count(b) == 0 for b in range(eng.bm.num_blocks))


def test_engine_seed_survives_a_preemption(tiny):
    eng, be = tiny
    p7 = SamplingParams(seed=7, **SAMPLED)
    want = _alone(eng, be, "list pods in prod", p7)
    eng.bm.reset_prefix_cache()
    items = [("list pods in prod", p7), ("get nodes -o wide", SamplingParams(max_new_tokens=8, ignore_eos=True))]
    outs = _staggered(eng, be, items, preempt=(0, 4))   # four tokens generated, then recomputed
    assert outs[0] == want


def test_engine_seeds_differ_and_unseeded_requests_draw_their_own(tiny):
    eng, be = tiny
    a = _alone(eng, be, "list pods in prod", SamplingParams(seed=7, **SAMPLED))
    b = _alone(eng, be, "list pods in prod", SamplingParams(seed=8, **SAMPLED))
    assert a != b
    s1, s2 = (Sequence(prompt_ids=[1], params=SamplingParams(**SAMPLED)) for _ in range(2))
    assert s1.sample_seed != s2.sample_seed and 0 <= s1.sample_seed <= M64
    assert Sequence(prompt_ids=[1], params=SamplingParams(seed=-1)).sample_seed == M64


def test_engine_temperature_zero_is_greedy_and_counts_no_sampled_step(tiny):
    eng, be = tiny
    greedy = SamplingParams(max_new_tokens=8, ignore_eos=True)
    want = _alone(eng, be, "describe deployment api", greedy)
    before = eng.runner.stats["sampled_steps"]
    for kw in (dict(top_k=3), dict(top_p=0.2), dict(seed=5), dict(top_k=2, top_p=0.5, seed=9)):
        p = SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=0.0, **kw)
        assert _alone(eng, be, "describe deployment api", p) == want
    assert eng.runner.stats["sampled_steps"] == before


def test_greedy_only_engine_counts_no_sampled_step():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=2048, max_model_len=256))
    be = EngineLLM(eng, max_new_tokens=4)
    eng.generate_blocking([be.prompt_ids(q) for q in ("list pods", "get nodes")], be.params, forced_prefix=be._forced)
    assert eng.runner.stats["sampled_steps"] == 0 and eng.runner.stats["decode_steps"] > 0


def test_async_paths_give_the_seeded_tokens(tiny):
    """launch_prefill_async, then chained launch_decode_async steps (position = num_generated + 1 while
    the previous token is still a placeholder) give the tokens of the synchronous path."""
    from ai_agent_kubectl_amd.engine.scheduler import Batch
    eng, be = tiny
    p7 = SamplingParams(seed=7, **SAMPLED)
    want = _alone(eng, be, "list pods in prod", p7)
    eng.bm.reset_prefix_cache()
    s = Sequence(prompt_ids=be.prompt_ids("list pods in prod"), params=p7, forced_prefix=list(be._forced))
    eng.scheduler.add(s)
    gather, eng.scheduler.gather_max_s = eng.scheduler.gather_max_s, 0.0   # everything is here
    try:
        batch = eng.scheduler.schedule()
    finally:
        eng.scheduler.gather_max_s = gather
    assert batch.seqs == [s]
    h = eng.runner.launch_prefill_async(batch)
    while True:
        nxt = None
        if s.num_generated + 1 < p7.max_new_tokens:
            eng.bm.ensure_capacity(s.block_table, s.total_len + 1)
            nxt = Batch([s], [1], is_decode=True)
            nh = eng.runner.launch_decode_async(nxt, chained=True)
        eng._apply(batch, eng.runner.collect(h))
        eng.scheduler.on_step_done(batch)
        if nxt is None:
            break
        batch, h = nxt, nh
    assert s.finished and s.output_ids == want


# ---------------- HTTP ----------------
def _client(be):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.config import Settings
    return TestClient(create_app(Settings(RATE_LIMIT="1000/minute", MODEL="tiny-llama"), backend=be))


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "list pods"}], "max_tokens": 6}


def test_http_seeded_sampling_repeats_and_validates(tiny):
    eng, be = tiny
    with _client(be) as c:
        before = eng.runner.stats["sampled_steps"]
        r1 = c.post("/v1/chat/completions", json=dict(BODY, temperature=0.8, seed=7, top_p=0.9, top_k=40))
        r2 = c.post("/v1/chat/completions", json=dict(BODY, temperature=0.8, seed=7, top_p=0.9, top_k=40))
        assert r1.status_code == 200 and r2.status_code == 200, (r1.text, r2.text)
        assert r1.json()["choices"][0]["message"]["content"] == r2.json()["choices"][0]["message"]["content"]
        assert eng.runner.stats["sampled_steps"] > before
        for bad in (dict(temperature=-1), dict(temperature=3), dict(top_p=0), dict(top_k=-1), dict(top_p=1.5)):
            assert c.post("/v1/chat/completions", json=dict(BODY, **bad)).status_code == 422, bad
        assert c.post("/v1/chat/completions", json=BODY).status_code == 200   # the fields stay optional


def test_http_sampling_under_tp_is_refused(tiny):
    eng, be = tiny
    eng.runner.tp_size = 2   # stands in for a tensor-parallel engine: submit refuses before anything runs
    try:
        with _client(be) as c:
            r = c.post("/v1/chat/completions", json=dict(BODY, temperature=0.8))
            assert r.status_code == 400 and "TP" in r.text
        with pytest.raises(ValueError):
            eng.submit([1, 2, 3], SamplingParams(temperature=0.5), lambda s: None)
    finally:
        eng.runner.tp_size = 1
