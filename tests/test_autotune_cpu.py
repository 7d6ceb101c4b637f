"""The decision rules of engine-start tuning (ops/autotune.py tune_*), on the CPU: a stub model of small
bf16 weights, `_time` replaced by scripted microseconds (the kernels are never run) and the plan file a
temp file.  Which kernel wins on an MI355X is the GPU suite's matter; what is done with the timings is this one's."""
import json
from types import SimpleNamespace

import pytest
import torch

from ai_agent_kubectl_amd import ops
from ai_agent_kubectl_amd.ops import autotune

T, F = True, False
QKV, SQ, W13 = (384, 256), (256, 256), (512, 256)   # wqkv | wo, w2 and the LM head | w13


def stub_model(w13_rows: int = 512, **attrs):
    w = lambda n, k: torch.zeros(n, k, dtype=torch.bfloat16)   # noqa: E731
    layers = [{"wqkv": w(*QKV), "wo": w(*SQ), "w13": w(w13_rows, 256), "w2": w(*SQ)} for _ in range(2)]
    return SimpleNamespace(layers=layers, W={"lm_head": w(*SQ)}, vocab_offset=0, cfg=SimpleNamespace(is_moe=False),
                           _local_comm=True, bf16_partials=True, **attrs)


class Clock:
    """Stands in for autotune._time: scripted microseconds in call order, `fn` never called.  A call
    beyond the script fails the test, so Clock() is also "must not be timed"."""

    def __init__(self, *us: float):
        self.us, self.calls = list(us), 0

    def __call__(self, fn, weights, reps=12, rounds=0):
        assert self.us, f"timing #{self.calls + 1} was not expected"
        self.calls += 1
        return self.us.pop(0)


@pytest.fixture(autouse=True)
def plan_file(tmp_path, monkeypatch):
    """Empty ops tables and default switches for the test, the plan file a temp path; all restored."""
    tables = (ops.GEMM_PLAN, ops.LM_HEAD_FUSED, ops.DECODE_SWIGLU_CFG, ops.PREFILL_PLAN)
    saved = [dict(t) for t in tables]
    for t in tables:
        t.clear()
    monkeypatch.setattr(ops, "LM_HEAD_FUSED_MIN_M", 64)
    monkeypatch.setattr(ops, "LM_HEAD_MODE", "auto")
    monkeypatch.setattr(ops, "DECODE_SWIGLU", "auto")
    monkeypatch.setattr(ops, "PREFILL_GEMM", "auto")
    monkeypatch.setattr(autotune, "BLAS_MARGIN", 0.15)
    monkeypatch.delenv("KA_PREFILL_MARGIN", raising=False)
    path = tmp_path / "plan.json"
    monkeypatch.setenv("KA_GEMM_PLAN_FILE", str(path))
    yield path
    for t, s in zip(tables, saved):
        t.clear()
        t.update(s)


def use_clock(monkeypatch, *us: float) -> Clock:
    clock = Clock(*us)
    monkeypatch.setattr(autotune, "_time", clock)
    return clock


# ---- LM head -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wins, min_m", [({1: F, 2: T, 4: F, 8: T}, 8), ({1: T, 2: T, 4: T, 8: T}, 1),
                                         ({1: F, 2: F, 4: F, 8: F}, 1 << 30)])
def test_lm_head_threshold_for_untimed_rows(monkeypatch, plan_file, wins, min_m):
    """Fused from the smallest bucket above which every timed bucket won.  `tune` mode neither reads the
    file (its entries say the opposite here) nor writes it."""
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    plan_file.write_text(json.dumps({"lm_head": {f"{M},256,256,0": [not f, 1.0, 2.0] for M, f in wins.items()}}))
    before = plan_file.read_bytes()
    clock = use_clock(monkeypatch, *[us for M in (1, 2, 4, 8) for us in (100.0, 90.0 if wins[M] else 120.0)])
    rep = autotune.tune_lm_head(stub_model(), (8, 1, 4, 2), None)
    assert ops.LM_HEAD_FUSED == wins and ops.LM_HEAD_FUSED_MIN_M == min_m == autotune._fused_min_m(wins)
    assert rep == {M: {"fused_us": 90.0 if f else 120.0, "unfused_us": 100.0, "fused": f} for M, f in wins.items()}
    assert clock.calls == 8 and plan_file.read_bytes() == before


@pytest.mark.parametrize("plan, fused", [(None, T), (("blas", 0, 0), T), (("gm", 1, 2), F)])
def test_lm_head_margin_only_over_hipblaslt(monkeypatch, plan, fused):
    """110 us fused against 100 us unfused: taken within BLAS_MARGIN (110 < 115) where the GEMM plan runs
    the LM head on hipBLASLt or has no entry, refused against a hand-written plan."""
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    if plan:
        ops.GEMM_PLAN[(4,) + SQ] = plan
    use_clock(monkeypatch, 100.0, 110.0)
    assert autotune.tune_lm_head(stub_model(), (4,), None)[4]["fused"] is fused
    assert ops.LM_HEAD_FUSED == {4: fused}


# ---- decode SwiGLU -------------------------------------------------------------------------------------
def test_decode_swiglu_cheapest_candidate_margin_and_zero_kept(monkeypatch):
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    assert ops.DECODE_SWIGLU_CFGS == (2, 3, 4, 5, 12) and ops.BIG_PLAN_MIN_M == 128
    ops.GEMM_PLAN[(16,) + W13] = ("gm", 1, 2)
    clock = use_clock(monkeypatch,
                      100.0, 120.0, 105.0, 130.0, 140.0, 150.0,        # M = 8: unfused, then cfgs 2, 3, 4, 5, 12
                      100.0, 120.0, 105.0, 130.0, 140.0, 150.0,        # M = 16: the same against a "gm" plan
                      100.0, 120.0, 105.0, 130.0, 140.0, 150.0, 80.0)  # M = 128: ... and DECODE_SWIGLU_BIG
    rep = autotune.tune_decode_swiglu(stub_model(), (128, 8, 16))
    assert clock.calls == 19 and not clock.us
    # 8: cfg 3 within the margin of an unplanned (hipBLASLt) gate_up; 16: no margin over a hand-written
    # plan, so unfused, stored as 0 and not left out; 128: gemm_big's epilogue is cheapest
    assert ops.DECODE_SWIGLU_CFG == {8: 3, 16: 0, 128: ops.DECODE_SWIGLU_BIG}
    assert rep == {8: {"cfg": 3, "fused_us": 105.0, "unfused_us": 100.0},
                   16: {"cfg": 0, "fused_us": 105.0, "unfused_us": 100.0},
                   128: {"cfg": ops.DECODE_SWIGLU_BIG, "fused_us": 80.0, "unfused_us": 100.0}}
    # an un-timed M answers from the next bucket up (CPU tensors stand in for device ones)
    monkeypatch.setattr(ops, "_ref", lambda t: False)
    w13 = stub_model().layers[0]["w13"]
    cfg_at = lambda M: ops.decode_swiglu_cfg(torch.zeros(M, 256, dtype=torch.bfloat16), w13)   # noqa: E731
    assert [cfg_at(M) for M in (4, 8, 12, 16, 100, 128, 200)] == [3, 3, 0, 0, ops.DECODE_SWIGLU_BIG,
                                                                  ops.DECODE_SWIGLU_BIG, 0]


@pytest.mark.parametrize("M, w13_rows, timings", [(64, 512, 6), (128, 512, 7), (128, 320, 6)])
def test_decode_swiglu_big_candidate(monkeypatch, M, w13_rows, timings):
    """gemm_big's SwiGLU epilogue is timed only from BIG_PLAN_MIN_M rows up and only where swiglu_gemm_ok
    (2I % 256): one timing more than unfused + DECODE_SWIGLU_CFGS."""
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    clock = use_clock(monkeypatch, *([100.0] * timings))
    autotune.tune_decode_swiglu(stub_model(w13_rows), (M,))
    assert clock.calls == timings and ops.DECODE_SWIGLU_CFG == {M: 2}   # all equal: the first candidate


# ---- prefill -------------------------------------------------------------------------------------------
def test_prefill_default_margin(monkeypatch):
    """gemm_big where it is within 2 % of hipBLASLt: 102.0 us against 100 us yes, 102.1 us no."""
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    n = len(ops.PREFILL_BUCKETS)
    clock = use_clock(monkeypatch, *([100.0, 102.0] * n + [100.0, 102.1] * n))   # hipBLASLt first; QKV, then O / down
    rep = autotune.tune_prefill(stub_model())
    assert clock.calls == 4 * n
    assert ops.PREFILL_PLAN == {(M,) + nk: nk == QKV for nk in (QKV, SQ) for M in ops.PREFILL_BUCKETS}
    assert rep == {**{f"{M},384,256": [T, 102.0, 100.0] for M in ops.PREFILL_BUCKETS},
                   **{f"{M},256,256": [F, 102.1, 100.0] for M in ops.PREFILL_BUCKETS}}


# ---- the plan file -------------------------------------------------------------------------------------
def full_sections() -> dict:
    return {"lm_head": {"2,256,256,0": [T, 9.0, 10.0], "8,256,256,0": [F, 12.0, 10.0]},
            "decode_swiglu": {"2,512,256": [4, 9.0, 10.0], "8,512,256": [0, 9.5, 10.0]},
            "prefill": {f"{M},{N},{K}": [N == 384, 50.0, 51.0] for (N, K) in (QKV, SQ) for M in ops.PREFILL_BUCKETS}}


def tune_sections(model, buckets, mask_bits=None):
    return (autotune.tune_lm_head(model, buckets, mask_bits), autotune.tune_decode_swiglu(model, buckets),
            autotune.tune_prefill(model))


def test_file_mode_takes_the_file_and_times_nothing(monkeypatch, plan_file):
    monkeypatch.setenv("KA_GEMM_PLAN", "file")
    plan_file.write_text(json.dumps(full_sections()))
    before = plan_file.read_bytes()
    use_clock(monkeypatch)
    lm, sw, pre = tune_sections(stub_model(), (2, 8))
    assert ops.LM_HEAD_FUSED == {2: T, 8: F} and ops.LM_HEAD_FUSED_MIN_M == 1 << 30
    assert ops.DECODE_SWIGLU_CFG == {2: 4, 8: 0}
    assert ops.PREFILL_PLAN == {(M,) + nk: nk == QKV for nk in (QKV, SQ) for M in ops.PREFILL_BUCKETS}
    # the saved times are the report's
    assert lm == {2: {"fused_us": 9.0, "unfused_us": 10.0, "fused": T}, 8: {"fused_us": 12.0, "unfused_us": 10.0, "fused": F}}
    assert sw == {2: {"cfg": 4, "fused_us": 9.0, "unfused_us": 10.0}, 8: {"cfg": 0, "fused_us": 9.5, "unfused_us": 10.0}}
    assert pre == full_sections()["prefill"]
    assert plan_file.read_bytes() == before


def test_file_mode_times_exactly_the_missing_key(monkeypatch, plan_file):
    monkeypatch.setenv("KA_GEMM_PLAN", "file")
    data = full_sections()
    del data["lm_head"]["8,256,256,0"], data["decode_swiglu"]["2,512,256"], data["prefill"]["3072,256,256"]
    plan_file.write_text(json.dumps(data))
    before = plan_file.read_bytes()
    model = stub_model()
    clock = use_clock(monkeypatch, 100.0, 90.0)                      # LM head M = 8: unfused, fused
    assert autotune.tune_lm_head(model, (2, 8), None)[8] == {"fused_us": 90.0, "unfused_us": 100.0, "fused": T}
    assert clock.calls == 2 and ops.LM_HEAD_FUSED == {2: T, 8: T} and ops.LM_HEAD_FUSED_MIN_M == 2
    clock = use_clock(monkeypatch, 100.0, 70.0, 60.0, 80.0, 80.0, 80.0)   # SwiGLU M = 2: unfused, five configurations
    assert autotune.tune_decode_swiglu(model, (2, 8))[2] == {"cfg": 3, "fused_us": 60.0, "unfused_us": 100.0}
    assert clock.calls == 6 and ops.DECODE_SWIGLU_CFG == {2: 3, 8: 0}
    clock = use_clock(monkeypatch, 100.0, 90.0)                      # prefill 3072 x (256, 256): hipBLASLt, gemm_big
    assert autotune.tune_prefill(model)["3072,256,256"] == [T, 90.0, 100.0]
    assert clock.calls == 2 and ops.PREFILL_PLAN[(3072,) + SQ] is T and ops.PREFILL_PLAN[(4096,) + SQ] is F
    assert plan_file.read_bytes() == before   # nothing is written in `file` mode, the new timings included


def test_write_mode_sections(monkeypatch, plan_file):
    """`write` re-times even what the file holds and merges the whole report into its section: key formats,
    value layouts, and everything else in the file survives."""
    monkeypatch.setenv("KA_GEMM_PLAN", "write")
    other = {"plans": {"8,256,256,plain": ["gm", 2, 5, 7.0, 9.0, 7.0]}, "device": "somewhere",
             "lm_head": {"8,256,256,0": [T, 1.0, 2.0], "4,256,256,1": [T, 1.0, 2.0]},
             "decode_swiglu": {"64,512,256": [2, 1.0, 2.0]}, "prefill": {"1024,64,64": [T, 1.0, 2.0]}}
    plan_file.write_text(json.dumps(other))
    n = len(ops.PREFILL_BUCKETS)
    clock = use_clock(monkeypatch, 100.0, 120.0,                               # LM head M = 4 (masked): not fused
                      100.0, 70.0, 60.0, 80.0, 80.0, 80.0,                     # SwiGLU M = 4: cfg 3
                      *([100.0, 90.04] * n + [100.0, 110.06] * n))             # prefill: QKV yes, O / down no
    tune_sections(stub_model(), (4,), mask_bits=torch.zeros(1, 8, dtype=torch.int32))
    assert clock.calls == 8 + 4 * n
    data = json.loads(plan_file.read_text())
    assert data["plans"] == other["plans"] and data["device"] == "somewhere"
    assert data["lm_head"] == {"8,256,256,0": [T, 1.0, 2.0], "4,256,256,1": [F, 120.0, 100.0]}
    assert data["decode_swiglu"] == {"64,512,256": [2, 1.0, 2.0], "4,512,256": [3, 60.0, 100.0]}
    assert data["prefill"] == {"1024,64,64": [T, 1.0, 2.0],
                               **{f"{M},384,256": [T, 90.0, 100.0] for M in ops.PREFILL_BUCKETS},
                               **{f"{M},256,256": [F, 110.1, 100.0] for M in ops.PREFILL_BUCKETS}}


# ---- decode GEMM plan (`file` mode: tuning what is missing enters TunableOp, a GPU matter) ---------------
def gemm_plan_file(plan_file, qkv_ctx: str = "plain") -> dict:
    plans = {f"{M},{N},{K},{ctx}": ["gm", M, 5, 7.0, 9.0, 7.0]
             for (N, K), ctx in ((QKV, qkv_ctx), (SQ, "norm-bf16"), (W13, "plain")) for M in (1, 8)}
    plan_file.write_text(json.dumps({"plans": plans}))
    return plans


def no_tuning(*args):
    raise AssertionError("tune_linear was not expected")


def test_gemm_plan_from_file(monkeypatch, plan_file):
    """O / down (and what shares their shape) are wanted with the norm's bf16 partials as consumer, the
    rest plain; a file that holds them all is the whole answer."""
    monkeypatch.setenv("KA_GEMM_PLAN", "file")
    gemm_plan_file(plan_file)
    monkeypatch.setattr(autotune, "tune_linear", no_tuning)
    assert autotune.tune_gemm_plan(stub_model(), [1, 8]) == {"from": str(plan_file)}
    assert ops.GEMM_PLAN == {(M,) + nk: ("gm", M, 5) for nk in (QKV, SQ, W13) for M in (1, 8)}


def test_gemm_plan_tunes_only_the_missing_entry(monkeypatch, plan_file):
    monkeypatch.setenv("KA_GEMM_PLAN", "file")
    plans = gemm_plan_file(plan_file)
    del plans["8,512,256,plain"]
    plan_file.write_text(json.dumps({"plans": plans}))
    before = plan_file.read_bytes()
    seen = []
    monkeypatch.setattr(autotune, "tune_linear", lambda *args: seen.append(args) or {"tuned": 1})
    model = stub_model()
    assert autotune.tune_gemm_plan(model, [1, 8]) == {"tuned": 1}
    (groups, Ms, norm_fed, bf16, consumers), = seen
    assert list(groups) == [W13] and all(a is b["w13"] for a, b in zip(groups[W13], model.layers))
    assert Ms == [8] and norm_fed == {SQ} and bf16 is True and consumers == {}
    assert (8,) + W13 not in ops.GEMM_PLAN and len(ops.GEMM_PLAN) == 5
    assert plan_file.read_bytes() == before


def test_gemm_plan_qkv_context_is_the_attention_consumer(monkeypatch, plan_file):
    """With a consumer from the runner and a model that fuses RoPE into a 128-wide attention, QKV is wanted
    (and would be timed) with that consumer; without either it is a plain shape."""
    monkeypatch.setenv("KA_GEMM_PLAN", "file")
    gemm_plan_file(plan_file, qkv_ctx="attn-bf16")
    seen = []
    monkeypatch.setattr(autotune, "tune_linear", lambda *args: seen.append(args) or {})
    consume = lambda qkv, M: qkv   # noqa: E731
    fused = dict(fuse_decode_rope=True, D=128, bf16_qkv_partials=True)
    assert autotune.tune_gemm_plan(stub_model(**fused), [1, 8], consume) == {"from": str(plan_file)} and not seen
    for model, consumer in ((stub_model(**fused), None), (stub_model(**{**fused, "D": 64}), consume)):
        autotune.tune_gemm_plan(model, [1, 8], consumer)
        groups, Ms, _, _, consumers = seen.pop()
        assert list(groups) == [QKV] and Ms == [1, 8] and consumers == {}


# ---- switches and the gate -----------------------------------------------------------------------------
def test_early_outs_clear_swiglu_and_prefill_but_not_lm_head(monkeypatch):
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    use_clock(monkeypatch)
    ops.LM_HEAD_FUSED[4], ops.DECODE_SWIGLU_CFG[4], ops.PREFILL_PLAN[(1024,) + SQ] = T, 2, T
    monkeypatch.setattr(ops, "LM_HEAD_MODE", "1")
    monkeypatch.setattr(ops, "DECODE_SWIGLU", "0")
    monkeypatch.setattr(ops, "PREFILL_GEMM", "blas")
    assert tune_sections(stub_model(), (4,)) == ({}, {}, {})
    assert ops.LM_HEAD_FUSED == {4: T} and ops.LM_HEAD_FUSED_MIN_M == 64
    assert ops.DECODE_SWIGLU_CFG == {} and ops.PREFILL_PLAN == {}
    ops.DECODE_SWIGLU_CFG[4] = 2
    monkeypatch.setattr(ops, "DECODE_SWIGLU", "auto")
    moe = stub_model()
    moe.cfg.is_moe = True
    assert autotune.tune_decode_swiglu(moe, (4,)) == {} and ops.DECODE_SWIGLU_CFG == {}


def test_tune_engine_on_a_cpu_model_tunes_nothing(monkeypatch, plan_file):
    monkeypatch.setenv("KA_GEMM_PLAN", "tune")
    use_clock(monkeypatch)
    monkeypatch.setattr(autotune, "tune_linear", no_tuning)
    ops.DECODE_SWIGLU_CFG[4], ops.PREFILL_PLAN[(1024,) + SQ] = 2, T
    assert autotune.tune_engine(stub_model(), [1, 8], None, lambda qkv, M: qkv) == {
        "gemm": {}, "lm_head": {}, "decode_swiglu": {}, "prefill": {}}
    assert ops.DECODE_SWIGLU_CFG == {4: 2} and ops.PREFILL_PLAN == {(1024,) + SQ: T} and not ops.GEMM_PLAN
    assert not plan_file.exists()
