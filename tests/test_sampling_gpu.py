"""csrc/sampling_stochastic.hip (`ops.sample`) against the float64 reference of tests/sampling_cases.py, and
the engine's sampled steps beside its captured greedy graphs.

Every case is one launch over rows that rotate through the modes of sampling_cases.MODES (greedy rows
inside the sampling batch, temperature only, top-k, top-p, both), so one reference per case serves
all the checks:
* temperature 0 rows: idx and val `torch.equal` to ops.masked_argmax;
* cut and kept: exactly the reference's on every row (they are bf16 values and integers) — the cases
  are chosen so that no top-p row's p is within 1e-3 of the total mass of a cumulative mass beside the
  cut (asserted), so no row is left out;
* the draw: idx equals the reference's on every row whose best two reference scores differ by more
  than 1e-3; at most 2 % of a case's rows may be left out (asserted);
* two launches give equal idx, val, cut and kept.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import sampling_cases as sc  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _lib():
    _hip.require()


def _dev(inp):
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return d


def _launch(d, cut=True):
    return ops.sample(d["logits"], d["bits"], d["midx"], d["temperature"], d["top_k"], d["top_p"], d["seed"],
                      d["position"], vocab_offset=d["off"], return_cut=cut)


def _check(inp, want, label):
    d = _dev(inp)
    idx, val, cut, kept = (t.cpu() for t in _launch(d))
    idx2, val2, cut2, kept2 = (t.cpu() for t in _launch(d))
    assert torch.equal(idx, idx2) and torch.equal(val, val2) and torch.equal(cut, cut2) and torch.equal(kept, kept2)
    s = sc.selectors(inp)
    near_p, near_gap = sc.side_conditions(inp, want)
    R = idx.shape[0]
    # temperature 0: the greedy kernel, bit for bit
    gi, gv = ops.masked_argmax(d["logits"], d["bits"], d["midx"], vocab_offset=d["off"])
    g = s["greedy"]
    assert torch.equal(idx[g], gi.cpu()[g]) and torch.equal(val[g], gv.cpu()[g]), label
    # the cuts: exact, no row left out
    assert not near_p.any(), (label, "a top-p row's p is within the margin of a cumulative mass: choose another seed")
    assert torch.equal(cut, want["cut"]), (label, cut, want["cut"])
    assert torch.equal(kept, want["kept"]), (label, kept, want["kept"])
    assert bool(torch.isinf(cut[s["nocut"]]).all())
    # the draw
    assert int(near_gap.sum()) <= 0.02 * R, (label, "too many rows with a score gap inside the margin")
    ok = s["sampled"] & ~near_gap
    print(f"{label}: rows {R}, sampled {int(s['sampled'].sum())}, left out {int(near_gap.sum())}, "
          f"idx mismatches {int((idx[ok] != want['idx'][ok]).sum())}, "
          f"max |val - ref| {float((val[ok].double() - want['val'][ok].double()).abs().max()) if ok.any() else 0:.3g}")
    assert torch.equal(idx[ok], want["idx"][ok]), label
    # the winning score, to the margin's derivation (want["val"] is the float64 score rounded to fp32)
    assert torch.allclose(val[ok], want["val"][ok], rtol=0, atol=1e-4), label
    off, V = inp["off"], inp["logits"].shape[1]
    assert bool(((idx >= off) & (idx < off + V)).all())


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: f"V{c[0]}-R{c[1]}-off{c[2]}-{'mask' if c[3] else 'nomask'}")
def test_sample_matches_float64_reference(case):
    inp, want = sc.build(case)
    _check(inp, want, str(case))


def test_sample_all_logits_equal():
    """One distinct value: both cuts sit on it and keep every allowed token; the token is the argmax
    of the noise alone."""
    inp, want = sc.build((32776, 3, 0, True), True)
    _check(inp, want, "all equal")
    assert bool((want["kept"] > 1).all())


@pytest.mark.parametrize("masked", [False, True])
def test_vocab_parallel_halves_merge_to_the_full_row(masked):
    """Temperature-only sampling on the two halves of a row, each with its own vocab_offset: the noise
    is indexed by the global id and the score comes back, so argmax_combine gives the full-row token."""
    V, R = 128256, 3
    h = V // 2
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(R, V, generator=g).to(sc.BF).to(DEV)
    bits = sc.make_mask(V, 0, 3).to(DEV) if masked else None
    midx = torch.tensor([0, -1, 1], dtype=torch.int32, device=DEV) if masked else None
    arr = (torch.tensor([0.7, 0.0, 1.25], device=DEV), torch.zeros(R, dtype=torch.int32, device=DEV),
           torch.ones(R, device=DEV), torch.tensor([11, 12, -13], dtype=torch.int64, device=DEV),
           torch.tensor([0, 5, 23], dtype=torch.int32, device=DEV))
    full_i, full_v = ops.sample(logits, bits, midx, *arr)
    parts = [ops.sample(logits[:, o:o + h].contiguous(), bits, midx, *arr, vocab_offset=o) for o in (0, h)]
    vals = torch.stack([p[1] for p in parts])
    idxs = torch.stack([p[0] for p in parts])
    assert torch.equal(ops.argmax_combine(vals, idxs), full_i)
    assert torch.equal(vals.max(dim=0).values, full_v)


def test_host_checks():
    lib = _hip.require()
    R = 2
    z = lambda dt: torch.zeros(R, dtype=dt, device=DEV)   # noqa: E731
    arr = (z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int64), z(torch.int32))
    with pytest.raises(RuntimeError):
        ops.sample(torch.zeros(R, 12, dtype=sc.BF, device=DEV), None, None, *arr)          # vocab % 8
    with pytest.raises(RuntimeError):
        ops.sample(torch.zeros(R, 16, dtype=sc.BF, device=DEV), None, None, *arr, vocab_offset=4)
    with pytest.raises(ValueError):
        ops.sample(torch.zeros(R, 16, dtype=sc.BF, device=DEV), None, None, arr[0], arr[1], arr[2], None, arr[4])
    logits = torch.zeros(R, 16, dtype=sc.BF, device=DEV)
    out_i, out_v = z(torch.int32), z(torch.float32)
    p = ops._p
    for missing in range(5):   # a null per-row array: hipErrorInvalidValue (1), nothing launched
        a = [p(t) for t in arr]
        a[missing] = None
        assert lib.ka_sample(p(out_i), p(out_v), None, None, p(logits), None, None, *a, R, 16, 0, 0, None, 1,
                             ops._stream()) == 1
    # a mask narrower than the global ids it is indexed by
    bits = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.sample(torch.zeros(R, 64, dtype=sc.BF, device=DEV), bits, z(torch.int32), *arr)


# ---------------- engine ----------------
@pytest.fixture(scope="module")
def eng_be():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    # llama3-8b-2l: the smallest preset the device kernels take (tiny-llama's head_dim 64 is CPU-only);
    # buckets 1 and 2 are the persistent decode kernel's, 4 the kernel chain's
    eng = build_engine(EngineOptions(model="llama3-8b-2l", device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=4096, max_model_len=256))
    eng.runner.capture_graphs()
    return eng, EngineLLM(eng, max_new_tokens=8)


def test_engine_sampled_steps_beside_the_greedy_graphs(eng_be):
    from ai_agent_kubectl_amd.engine.sequence import SamplingParams
    eng, be = eng_be
    st = eng.runner.stats
    assert eng.runner.graphs and st["sampled_steps"] == 0
    p7 = SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=0.9, top_k=50, top_p=0.95, seed=7)
    greedy = SamplingParams(max_new_tokens=8, ignore_eos=True)
    ids = be.prompt_ids("list pods in prod")
    a = eng.generate_blocking([ids], p7, forced_prefix=be._forced)[0].output_ids
    n1 = st["sampled_steps"]
    assert n1 > 0
    eng.bm.reset_prefix_cache()   # both runs prefill the whole prompt: the same kernels, the same logits
    b = eng.generate_blocking([ids], p7, forced_prefix=be._forced)[0].output_ids
    assert a == b and st["sampled_steps"] > n1
    # queued ahead of the readback (position = num_generated + 1): the same tokens
    eng.bm.reset_prefix_cache()
    assert sc.chain_async(eng, sc.new_sequence(be, "list pods in prod", p7)) == a
    # three rows (bucket 4, the kernel chain): the same tokens in two runs
    many = [be.prompt_ids(q) for q in ("list pods in prod", "get nodes -o wide", "describe svc api")]
    runs = []
    for _ in range(2):
        eng.bm.reset_prefix_cache()
        runs.append([s.output_ids for s in eng.generate_blocking(many, p7, forced_prefix=be._forced)])
    assert runs[0] == runs[1]
    # a greedy-only run afterwards still replays the graphs
    n2, r2 = st["sampled_steps"], st["graph_replays"]
    eng.bm.reset_prefix_cache()
    g1 = eng.generate_blocking([ids], greedy, forced_prefix=be._forced)[0].output_ids
    assert st["graph_replays"] > r2 and st["sampled_steps"] == n2
    # and temperature 0 with cuts and a seed is that greedy output, on the graphs too
    p0 = SamplingParams(max_new_tokens=8, ignore_eos=True, temperature=0.0, top_k=3, top_p=0.5, seed=1)
    eng.bm.reset_prefix_cache()
    assert eng.generate_blocking([ids], p0, forced_prefix=be._forced)[0].output_ids == g1
    assert st["sampled_steps"] == n2
