"""Full-depth numerics of the model the headline runs: Llama-3-8B, all 32 layers (VERDICT r4 missing #3).

The 2-layer tests in test_model_gpu.py pin every kernel; these pin what only shows at full depth — the
persistent batch-1 kernel's grid barriers and layer-table walk over 32 layers, cache offsets of the
late layers, and the growth of bf16 error over 32 residual updates — against the same forward through
the fp32 torch references (`ops.force_reference`) on the same random-init weights:

* a >= 1024-row prefill step through the prefill kernels, with the logits error recorded at depth
  2 / 8 / 16 / 32 (the model's first d layers, then the final norm and LM head);
* 8 decode steps at B = 1 and at B = 2 (the persistent all-layers kernel, eagerly and as the captured
  graph);
* 8 decode steps at B = 256 (the kernel chain of the headline's decode bucket, eagerly and as the
  captured graph).
Each decode step compares the HIP forward with the reference forward on clones of the same KV cache
(re-based every step), and the graph replay's sampled tokens with the eager step's.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine  # noqa: E402
from ai_agent_kubectl_amd.engine.scheduler import Batch  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402
from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM  # noqa: E402
from ai_agent_kubectl_amd.models.llama import AttnMeta  # noqa: E402

QUERIES = ["list all pods", "show services in namespace prod", "scale web to 3 replicas",
           "get nodes with labels", "describe deployment api", "logs of pod api-1"]
DEPTHS = (2, 8, 16, 32)
# bounds for the full model (measured values are printed and kept in profiles/r5/full_depth/):
# logits cosine vs fp32 at every depth, and max |dlogit| relative to the reference logits' spread.
# bf16 rounding errors of independent layers add like a random walk (first measurement: rel 0.049 /
# 0.107 / 0.169 / 0.266 at depth 2 / 8 / 16 / 32, x1.4-1.6 per doubling); the growth bound allows
# 2x that sqrt(depth) walk and fails on the linear or exponential growth of a defect at depth.
COS_MIN = 0.99
REL_MAX = 0.5
REL2_MAX = 0.1   # depth 2 (measured 0.049): a wrong kernel shows here before any growth argument


def _growth_ok(rows):
    rel2 = rows[0][3]
    return all(rel <= 2.0 * rel2 * (d / rows[0][0]) ** 0.5 + 1e-3 for d, _, _, rel in rows)


@pytest.fixture(scope="module")
def eng():
    opts = EngineOptions(model="llama3-8b", device="cuda", max_batch=256, graph_buckets=(1, 2, 256),
                         kv_cache_tokens=49152, max_model_len=1024, max_batched_tokens=16384, use_graphs=True)
    e = build_engine(opts)
    assert len(e.runner.model.layers) == 32
    e.runner.capture_graphs()
    yield e
    del e
    torch.cuda.empty_cache()


def _cmp(lg, lg_ref):
    lg, lg_ref = lg.float(), lg_ref.float()
    cos = torch.nn.functional.cosine_similarity(lg, lg_ref, dim=-1).min().item()
    err = (lg - lg_ref).abs().max().item()
    rel = err / lg_ref.std().item()
    return cos, err, rel


def _prefill_meta(r, batch):
    host = torch.from_numpy(r._pack_prefill(batch)).cuda()
    T, S, mb = batch.num_tokens, len(batch.seqs), r.max_blocks
    o = 3 * T
    meta = AttnMeta(positions=host[T:2 * T], slot_mapping=host[2 * T:3 * T],
                    block_tables=host[o + 4 * S + 1:o + 4 * S + 1 + S * mb].view(S, mb),
                    ctx_lens=host[o + S + 1:o + 2 * S + 1], logits_indices=host[o + 3 * S + 1:o + 4 * S + 1].long(),
                    is_decode=False, q_starts=host[o:o + S + 1], max_q_len=max(batch.num_query))
    return host[:T], meta


def test_full_depth_prefill_error_growth(eng):
    """A >= 1024-row prefill step: HIP vs fp32 logits at depth 2 / 8 / 16 / 32."""
    be = EngineLLM(eng, max_new_tokens=8)
    r, m = eng.runner, eng.runner.model
    queries = [f"{q} in namespace team-{i} sorted by creation time" for i, q in enumerate(QUERIES * 2)]
    seqs = [Sequence(prompt_ids=be.prompt_ids(q), params=be.params) for q in queries]
    for s in seqs:
        s.block_table, _, s.block_hashes = eng.bm.allocate_prompt(s.all_ids)
    batch = Batch(seqs, [s.total_len for s in seqs], is_decode=False, prefill_seqs=seqs)
    assert batch.num_tokens >= 1024, batch.num_tokens
    full = list(m.layers)
    rows = []
    try:
        with torch.inference_mode():
            ids, meta = _prefill_meta(r, batch)
            for d in DEPTHS:
                m.layers = full[:d]
                lg = m.logits(m.forward(ids, meta, r.k_cache, r.v_cache))
                with ops.force_reference():
                    lg_ref = m.logits(m.forward(ids, meta, r.k_cache, r.v_cache))
                rows.append((d,) + _cmp(lg, lg_ref))
    finally:
        m.layers = full
        for s in seqs:
            eng.bm.free_table(s.block_table)
    print("\nprefill %d rows: depth, min logits cosine, max |dlogit|, max |dlogit| / std(ref logits)" % batch.num_tokens)
    for d, cos, err, rel in rows:
        print(f"  depth {d:2d}: cos {cos:.5f}  max|d| {err:.4f}  rel {rel:.4f}")
    for d, cos, err, rel in rows:
        assert cos > COS_MIN, rows
        assert rel < REL_MAX, rows
    assert rows[0][3] < REL2_MAX, rows
    assert _growth_ok(rows), rows


def _decode_run(eng, B, steps=8, graph=True):
    """B sequences prefilled, then `steps` decode steps: eager HIP vs the fp32 truth on cloned caches
    (ops.force_reference(fp32=True): reference ops with fp32 activations and residual stream; before
    round 6 this reference ran the persistent HIP kernel itself at B <= 2, which hid its error),
    and the captured graph of bucket B (which writes the real cache) vs the eager step's tokens.  Per
    step: (logits cosine, max |dlogit|, rel, greedy-token agreement), the agreement being the fraction
    of rows whose HIP token (the SAFE_DECODE-masked argmax the engine samples, `temperature=0`,
    app.py:109) equals the fp32 reference's masked argmax on the same cache.  graph=False: no graph
    replay (the eager step writes the real cache), for model settings the captured graph does not have."""
    be = EngineLLM(eng, max_new_tokens=40, ignore_eos=True)
    params = SamplingParams(max_new_tokens=40, ignore_eos=True)
    sch, r, m = eng.scheduler, eng.runner, eng.runner.model
    sch.prefill_max_wait_s = 0.0
    sch.gather_max_s = 0.0
    sch.hold_steps = 0
    out = []
    for s in list(sch.running) + list(sch.waiting):   # whatever an earlier (failed) test left behind
        sch.abort(s)
    try:
        _decode_steps(eng, B, steps, graph, out, be, params)
    finally:
        for s in list(sch.running) + list(sch.waiting):   # the next test starts with an empty scheduler
            sch.abort(s)
    return out


def _decode_steps(eng, B, steps, graph, out, be, params):
    sch, r, m = eng.scheduler, eng.runner, eng.runner.model
    with torch.inference_mode():
        for i in range(B):
            sch.add(Sequence(prompt_ids=be.prompt_ids(QUERIES[i % len(QUERIES)] + f" #{i}"), params=params,
                             forced_prefix=list(be._forced)))
        while sch.waiting:
            b = sch.schedule()
            eng._apply(b, r.execute(b))
            sch.on_step_done(b)
        assert len(sch.running) == B
        g = r.graphs[B]
        for step in range(steps):
            batch = sch.schedule()
            assert batch.is_decode and len(batch.seqs) == B
            r._pack_decode(batch, B)
            n = r._off["bt"] + B * r.max_blocks
            r.d_stage[:n].copy_(r.h_stage[:n])
            meta = AttnMeta(positions=r._view("pos", B), slot_mapping=r._view("slots", B),
                            block_tables=r._view("bt", B), ctx_lens=r._view("ctx", B),
                            logits_indices=r.d_logits_idx[:B], is_decode=True)
            ids = r._view("ids", B)
            mask = r._view("mask", B) if r.mask_bits is not None else None
            kr, vr = r.k_cache.clone(), r.v_cache.clone()
            with ops.force_reference(fp32=True):   # the fp32 truth (activations / residual in fp32)
                h_ref = m.forward(ids, meta, kr, vr)
                lg_ref = m.logits(h_ref).float()[:B]
                tok_ref = m.sample(h_ref, r.mask_bits, mask)[:B].tolist()
            del kr, vr, h_ref
            if graph:
                kc, vc = r.k_cache.clone(), r.v_cache.clone()
            else:
                kc, vc = r.k_cache, r.v_cache
            h = m.forward(ids, meta, kc, vc)
            lg = m.logits(h).float()[:B]
            tok = m.sample(h, r.mask_bits, mask)[:B].tolist()
            if B <= 2:
                torch.cuda.synchronize()
                assert m.persistent_err() == 0
            del kc, vc
            agree = sum(a == b for a, b in zip(tok, tok_ref)) / B
            # every disagreement's fp32 logit margin: how far the fp32 truth prefers its token over the
            # HIP token (both allowed by the mask); a near-tie is smaller than the step's logit error
            gap = max([float(lg_ref[i, tok_ref[i]] - lg_ref[i, tok[i]]) for i in range(B) if tok[i] != tok_ref[i]],
                      default=0.0)
            out.append(_cmp(lg, lg_ref) + (agree, gap))
            if graph:
                g.replay()   # the real cache gets this step's keys / values from the graph
                torch.cuda.synchronize()
                assert r.d_out[:B].tolist() == tok, step
            if B <= 2:
                assert m.persistent_err() == 0
            eng._apply(batch, tok)
            sch.on_step_done(batch)


@pytest.mark.parametrize("B", [1, 2])
def test_persistent_decode_repeatable_under_alternating_launches(eng, B):
    """VERDICT r5 next #1 for csrc/decode_persistent.hip: the same decode step (same cache slot, so the
    KV append is idempotent) launched again and again, each launch right after an unrelated GEMM, must
    give the bitwise-same hidden states: the kernel has one fixed summation order, so a weight piece
    read from its LDS ring before it landed shows as a differing repeat.  The streams wait for their
    pieces with vmcnt(0) only (each ring's two drained halves)."""
    be = EngineLLM(eng, max_new_tokens=40, ignore_eos=True)
    params = SamplingParams(max_new_tokens=40, ignore_eos=True)
    sch, r, m = eng.scheduler, eng.runner, eng.runner.model
    sch.prefill_max_wait_s = 0.0
    sch.gather_max_s = 0.0
    other = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)
    wo = (torch.randn(4096, 4096, device="cuda") / 64).to(torch.bfloat16)
    reps = int(__import__("os").environ.get("KA_PD_STRESS_REPS", "150"))
    with torch.inference_mode():
        for i in range(B):
            sch.add(Sequence(prompt_ids=be.prompt_ids(QUERIES[i] + f" again #{i}"), params=params,
                             forced_prefix=list(be._forced)))
        while sch.waiting:
            b = sch.schedule()
            eng._apply(b, r.execute(b))
            sch.on_step_done(b)
        batch = sch.schedule()
        assert batch.is_decode and len(batch.seqs) == B and m.persistent_ok(B)
        r._pack_decode(batch, B)
        n = r._off["bt"] + B * r.max_blocks
        r.d_stage[:n].copy_(r.h_stage[:n])
        meta = AttnMeta(positions=r._view("pos", B), slot_mapping=r._view("slots", B),
                        block_tables=r._view("bt", B), ctx_lens=r._view("ctx", B),
                        logits_indices=r.d_logits_idx[:B], is_decode=True)
        ids = r._view("ids", B)
        first = m.forward(ids, meta, r.k_cache, r.v_cache).clone()
        bad = torch.zeros(reps, dtype=torch.int64, device="cuda")
        for i in range(reps):
            torch.nn.functional.linear(other, wo)
            bad[i] = (m.forward(ids, meta, r.k_cache, r.v_cache) != first).sum()
        torch.cuda.synchronize()
        assert m.persistent_err() == 0
        for s in list(sch.running):
            sch.abort(s)
    nbad = int((bad > 0).sum())
    print(f"\nB={B} persistent decode: {nbad} of {reps} repeats differ from the first launch")
    assert nbad == 0


# greedy-token agreement with the fp32 reference, mean over the 8 steps (VERDICT r5 missing #5): the
# token is what temperature=0 returns, so this pins the parity of generated tokens, not only logits.
# Random-init weights give flat logits (near-ties are common), so the bound is a rate, not equality;
# measured values: profiles/r6/token_parity/.
AGREE_MIN = {1: 0.75, 2: 0.75, 256: 0.8}


def _report(name, res):
    print(f"\n{name}: per-step (cos, max|d|, rel, token agreement, largest fp32 margin of a disagreement):",
          [tuple(round(v, 4) for v in x) for x in res])
    agree = sum(x[3] for x in res) / len(res)
    print(f"{name}: mean greedy-token agreement with fp32 = {agree:.4f}, max rel = {max(x[2] for x in res):.4f}, "
          f"largest fp32 logit margin of a disagreeing row = {max(x[4] for x in res):.4f} "
          f"(max |dlogit| {max(x[1] for x in res):.4f})")
    # every disagreement is a near-tie of the fp32 model: the HIP logits rank the two tokens the other
    # way round, so the fp32 margin is at most the logit error of both (2 max |dlogit|)
    assert all(x[4] <= 2 * x[1] + 1e-3 for x in res), res
    return agree


def test_full_depth_decode_b1_persistent(eng):
    m = eng.runner.model
    assert m.persistent_ok() and eng.runner.graph_persistent.get(1)
    res = _decode_run(eng, 1)
    agree = _report("B=1 persistent decode, 32 layers", res)
    for cos, err, rel, _, _ in res:
        assert cos > COS_MIN and rel < REL_MAX, res
    assert agree >= AGREE_MIN[1], res


def test_full_depth_decode_b2_persistent(eng):
    """The persistent kernel at B = 2 (both sequences' rows against one weight stream, a leader per
    sequence and KV group) over the full 32 layers."""
    m = eng.runner.model
    assert m.persistent_ok(2) and eng.runner.graph_persistent.get(2)
    res = _decode_run(eng, 2)
    agree = _report("B=2 persistent decode, 32 layers", res)
    for cos, err, rel, _, _ in res:
        assert cos > COS_MIN and rel < REL_MAX, res
    assert agree >= AGREE_MIN[2], res


def test_full_depth_decode_b256_graph(eng):
    res = _decode_run(eng, 256)
    agree = _report("B=256 decode chain, 32 layers", res)
    for cos, err, rel, _, _ in res:
        assert cos > COS_MIN and rel < REL_MAX, res
    assert agree >= AGREE_MIN[256], res


def test_full_depth_decode_b2_kernel_chain(eng):
    """Attribution: B = 2 through the kernel chain the large buckets use instead of
    the persistent kernel (eagerly), so the chain and the persistent kernel are compared at the same
    rows: the chain rounds the residual stream and every projection output to bf16 (as the fp32
    reference does), the persistent kernel keeps the residual in fp32."""
    m = eng.runner.model
    saved = m.persistent
    m.persistent = False
    try:
        res = _decode_run(eng, 2, graph=False)
    finally:
        m.persistent = saved
    agree = _report("B=2 decode kernel chain (no persistent kernel), 32 layers", res)
    for cos, err, rel, _, _ in res:
        assert cos > COS_MIN and rel < REL_MAX, res
    assert agree >= AGREE_MIN[2], res


def test_full_depth_decode_b256_fp32_partials(eng):
    """Attribution of the B = 256 error: the same chain with the split-K partials
    of O / down (KA_BF16_PARTIALS) and QKV (KA_BF16_QKV_PARTIALS) kept in fp32, eagerly (the captured
    graph has the bf16 slabs).  Prints rel and agreement for the A/B against the bf16-partials run."""
    m = eng.runner.model
    saved = (m.bf16_partials, m.bf16_qkv_partials)
    m.bf16_partials = m.bf16_qkv_partials = False
    try:
        res = _decode_run(eng, 256, graph=False)
    finally:
        m.bf16_partials, m.bf16_qkv_partials = saved
    agree = _report("B=256 decode chain, fp32 split-K partials, 32 layers", res)
    for cos, err, rel, _, _ in res:
        assert cos > COS_MIN and rel < REL_MAX, res
    assert agree >= AGREE_MIN[256], res
