"""csrc/lora.hip (`ops.lora_add`) against ops/reference.py: exact probes at the shapes that straddle the kernel's
tiles, real-valued data at the real projection shapes against float64 with the derived per-element bound, the
launcher's return codes, and the adapter route of the model and the engine on llama3-8b-2l."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from ai_agent_kubectl_amd.ops import reference as ref  # noqa: E402
from tests import lora_cases as lc  # noqa: E402

DEV = "cuda"
HIP_INVALID = 1   # hipErrorInvalidValue


@pytest.fixture(autouse=True, scope="module")
def _lib():
    assert ops.lora_geometry() == (lc.TILE_ROWS, lc.TILE_N)   # the geometry the cases straddle is the kernel's


def _dev(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _run(c, y):
    return ops.lora_add(y, c["x"], c["row_adapter"], c["A"], c["B"], c["scale"], c["seg"])


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("T,K,widths,R,r", lc.EXACT_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_exact_probe_matches_the_reference_bit_for_bit(T, K, widths, R, r):
    cpu = lc.exact_case(T, K, widths, R, r)
    t_max = (cpu["x"].float().abs() @ cpu["A"].float().abs().flatten(0, 2).T).max().item()
    assert t_max <= 256                                      # t is exact in bf16
    assert (cpu["row_adapter"] == 2).any() and (T < 3 or (cpu["row_adapter"] < 0).any())
    want = ref.lora_add(cpu["y"].clone(), cpu["x"], cpu["row_adapter"], cpu["A"], cpu["B"], cpu["scale"], cpu["seg"])
    c = _dev(cpu)
    got = _run(c, c["y"].clone())
    again = _run(c, c["y"].clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(again)), "two launches differ"
    bad = (_bits(got.cpu()) != _bits(want)).nonzero()
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    none = cpu["row_adapter"] < 0
    assert (_bits(got.cpu())[none] == lc.SENTINEL).all()      # rows of -1 keep the sentinel
    a1 = cpu["row_adapter"] == 1                              # adapter 1's first segment has scale 0
    assert torch.equal(_bits(got.cpu())[a1, :widths[0]], _bits(cpu["y"])[a1, :widths[0]])
    assert not torch.equal(_bits(got.cpu()), _bits(cpu["y"]))


# the four projections of Llama-3-8B: (K, widths)
REAL_SHAPES = {"wqkv": (4096, (4096, 1024, 1024)), "wo": (4096, (4096,)), "w13": (4096, (14336, 14336)),
               "w2": (14336, (4096,))}


@pytest.mark.parametrize("T", (1, 256, 1040))
@pytest.mark.parametrize("name", sorted(REAL_SHAPES))
def test_real_data_within_the_derived_bound(name, T):
    K, widths = REAL_SHAPES[name]
    c = lc.real_case(T, K, widths, device=DEV)
    y_ref, bound = lc.float64_truth(c)
    got = _run(c, c["y"].clone())
    err = (got.double() - y_ref).abs()
    touched = bound > 0
    ratio = (err[touched] / bound[touched]).max().item()
    print(f"lora_add {name} T={T}: largest error / bound = {ratio:.4f} over {int(touched.sum())} elements")
    assert touched.any() and (err <= bound).all(), ratio     # every element; untouched ones: error 0 = bound 0
    assert torch.equal(_bits(got)[~touched], _bits(c["y"])[~touched])


def test_launcher_refuses_bad_arguments_and_launches_nothing():
    lib = _hip.require()
    c = _dev(lc.exact_case(3, 64, (16, 16, 16), 16, 8))
    y = c["y"].clone()
    T, N, K, S, R, n = 3, 48, 64, 3, 16, 3
    ws = torch.zeros(int(lib.ka_lora_splits(T, S, K)) * T * S * R, dtype=torch.float32, device=DEV)
    seg = (ctypes.c_int * 4)(*c["seg"])
    ptrs = [y.data_ptr(), c["x"].data_ptr(), c["row_adapter"].data_ptr(), c["A"].data_ptr(), c["B"].data_ptr(),
            c["scale"].data_ptr(), seg, ws.data_ptr()]
    stream = torch.cuda.current_stream().cuda_stream

    def call(p, T=T, N=N, K=K, S=S, R=R, n=n):
        return lib.ka_lora_add(*p, T, N, K, S, R, n, stream)

    for i in range(len(ptrs)):
        assert call(ptrs[:i] + [None] + ptrs[i + 1:]) == HIP_INVALID, i
    assert call(ptrs, K=96) == HIP_INVALID                    # K % 64
    assert call(ptrs, N=56) == HIP_INVALID                    # N % 16 (and seg[S] != N)
    assert call(ptrs, R=8) == HIP_INVALID
    assert call(ptrs, n=9) == HIP_INVALID
    for bad in ((0, 24, 32, 48), (0, 16, 16, 48), (16, 32, 48, 48), (0, 16, 32, 64)):
        assert call(ptrs[:6] + [(ctypes.c_int * 4)(*bad)] + ptrs[7:]) == HIP_INVALID, bad
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(c["y"]))               # nothing ran
    assert call(ptrs) == 0
    torch.cuda.synchronize()
    want = ref.lora_add(c["y"].cpu().clone(), *(c[k].cpu() for k in ("x", "row_adapter", "A", "B", "scale")), c["seg"])
    assert torch.equal(_bits(y.cpu()), _bits(want))


# ---------------- the model and the engine on llama3-8b-2l ----------------
from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine  # noqa: E402
from ai_agent_kubectl_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402
from ai_agent_kubectl_amd.models import lora as mlora  # noqa: E402
from ai_agent_kubectl_amd.models.config import get_config  # noqa: E402

MODEL = "llama3-8b-2l"
CFG = get_config(MODEL)
ALL = tuple(mlora.MODULES)
# delta = scale B A has entries of std 2 * 0.04 * 0.04 * sqrt(16) = 0.013 beside the base weights' 0.02
ADAPTERS = {"kube": (16, 32, ALL, 11), "alt": (16, 32, ALL, 12)}
PROMPTS = ("list all pods in the prod namespace", "show the logs of the api deployment", "get nodes",
           "describe the ingress of the web service")
ATOL, RTOL = 0.1, 0.05   # tests/test_model_gpu.py's forward tolerance


@pytest.fixture(scope="module")
def peft(tmp_path_factory):
    root = tmp_path_factory.mktemp("adapters")
    out = {}
    for name, (r, alpha, mods, seed) in ADAPTERS.items():
        t = lc.peft_tensors(CFG, r, mods, seed=seed, std_a=0.04, std_b=0.04)
        out[name] = (lc.write_peft_dir(root / name, t, r, alpha, mods), t, lc.lora_scale(r, alpha))
    return out, ",".join(f"{n}={d}" for n, (d, _, _) in out.items())


def _engine(graphs, **kw):
    eng = build_engine(EngineOptions(model=MODEL, device="cuda", max_batch=4, graph_buckets=(1, 2, 4),
                                     kv_cache_tokens=8192, max_model_len=256, use_graphs=graphs, **kw))
    if graphs:
        eng.runner.capture_graphs(autotune=False)
    sch = eng.scheduler
    sch.prefill_max_wait_s = sch.gather_max_s = 0.0
    sch.hold_steps = 0
    return eng


def _params(adapter=None, n=5):
    return SamplingParams(max_new_tokens=n, ignore_eos=True, safe_decode=False, adapter=adapter)


def _step(eng):
    batch = eng.scheduler.schedule()
    eng._apply(batch, eng.runner.execute(batch))
    eng.scheduler.on_step_done(batch)
    return batch


def _generate(eng, prompts, adapters, n=5):
    eng.bm.reset_prefix_cache()
    seqs = [Sequence(prompt_ids=list(p), params=_params(a, n)) for p, a in zip(prompts, adapters)]
    for s in seqs:
        eng.scheduler.add(s)
    while not all(s.finished for s in seqs):
        _step(eng)
    return [list(s.output_ids) for s in seqs]


def test_adapter_route_hip_vs_reference(peft):
    """Every step of two small runs (a prefill, a mixed step, decode at B = 1 and B = 3 padded to the bucket of 4,
    rows of two adapters and of none) goes through the HIP route and, on a copy of the KV cache, through the same
    route under ops.force_reference(); the reference is also taken without the adapters to show that they matter."""
    import dataclasses
    eng = _engine(False, lora_adapters=peft[1])
    m = eng.runner.model
    orig = m.forward
    seen = []

    def both(ids, meta, kc, vc):
        assert meta.adapter is not None and meta.adapter.dtype == torch.int32 and meta.adapter.shape == ids.shape
        with ops.force_reference():
            h_ref = orig(ids, meta, kc.clone(), vc.clone())
            h_base = orig(ids, dataclasses.replace(meta, adapter=None), kc.clone(), vc.clone())
        h = orig(ids, meta, kc, vc)
        rows = meta.adapter if meta.is_decode else meta.adapter[meta.logits_indices]
        n = int(meta.ctx_lens.gt(0).sum())
        kind = "decode" if meta.is_decode else "mixed" if meta.num_decode else "prefill"
        seen.append((kind, n, rows[:n].tolist(), h[:n].float(), h_ref[:n].float(), h_base[:n].float()))
        return h

    m.forward = both
    ids = [eng.tokenizer.encode(p) for p in PROMPTS]
    with torch.inference_mode():
        _generate(eng, ids[:1], [0], n=3)                      # prefill, decode at B = 1
        eng.bm.reset_prefix_cache()
        seqs = [Sequence(prompt_ids=list(p), params=_params(a, 4)) for p, a in zip(ids[1:], (0, None, 1))]
        for s in seqs[:2]:
            eng.scheduler.add(s)
        _step(eng)                                        # prefill of two
        eng.scheduler.add(seqs[2])
        while not all(s.finished for s in seqs):          # a mixed step, then decode at B = 3
            _step(eng)
    m.forward = orig
    kinds = {(k, n) for k, n, *_ in seen}
    assert {("prefill", 1), ("decode", 1), ("prefill", 2), ("mixed", 3), ("decode", 3)} <= kinds, kinds
    moved = 0.0
    for kind, n, rows, h, h_ref, h_base in seen:
        torch.testing.assert_close(h, h_ref, atol=ATOL, rtol=RTOL, msg=lambda s: f"{kind} {n} {rows}: {s}")
        live = torch.tensor([a >= 0 for a in rows], device=h.device)
        assert live.any()
        excess = ((h_ref - h_base).abs() - 4 * (ATOL + RTOL * h_base.abs()))[live]
        moved = max(moved, excess.max().item())
        assert excess.max().item() > 0, (kind, n, "the adapter moves the hidden state by less than 4x the tolerance")
    print(f"adapter route: {len(seen)} steps, the adapters move the reference by 4 tol + {moved:.3f} at the most")
    assert eng.runner.stats["lora_steps"] == len(seen)


def test_engine_adapter_tokens_and_graphs_for_base_batches(peft):
    from tests.virtual_tp import assert_same_or_near_tie
    eng = _engine(True, lora_adapters=peft[1])
    prompts = [eng.tokenizer.encode(p) for p in PROMPTS]
    with torch.inference_mode():
        base = _generate(eng, prompts, [None] * 4)
        assert eng.runner.stats["lora_steps"] == 0 and eng.runner.stats["graph_replays"] > 0
        got = _generate(eng, prompts, [0, None, 1, 0])
        steps = eng.runner.stats["lora_steps"]
        assert steps > 0
        # the merged-weight engine through the reference ops: what a CPU engine computes
        merged = _engine(False)
        mm = merged.runner.model
        mm.W = lc.merged_weights(mm.W, CFG, peft[0]["kube"][1], peft[0]["kube"][2])
        mm.layers = [mm._layer(i) for i in range(CFG.num_layers)]
        kube = [0, 3]
        with ops.force_reference():
            want = [_generate(merged, [prompts[i]], [None])[0] for i in kube]
            assert_same_or_near_tie(merged, [prompts[i] for i in kube], want, [got[i] for i in kube])
        assert any(got[i] != base[i] for i in kube), "the adapter does not matter: the comparison shows nothing"
        # a base-only batch afterwards: the captured graphs again, no adapter step
        replays = eng.runner.stats["graph_replays"]
        again = _generate(eng, prompts, [None] * 4)
        assert again == base
        assert eng.runner.stats["graph_replays"] > replays and eng.runner.stats["lora_steps"] == steps
