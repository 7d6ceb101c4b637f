"""GEMM plan autotuning for the decode path.

For every projection shape (N, K) of the loaded model and every decode batch bucket M, time the
hand-written weight-streaming kernel at a few split-K factors against hipBLASLt (`F.linear`) on the
model's *own* weights, rotating over layers so each call streams from HBM as in a real step, and
record the winner in `ops.GEMM_PLAN`.  Done once at engine start (before hipGraph capture), so the
captured graphs contain the fastest kernel per shape.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops
from . import (BIG_PLAN_MIN_M, GEMM_PLAN, SKINNY_MAX_M, TILE_MAX_M, big_gemm_ok, gm_shape, linear, linear_big,
               linear_gm, linear_rows, rmsnorm, rows_ok, skinny_split)

logger = logging.getLogger("app.engine")

# TunableOp results for the decode GEMM shapes on MI355X (ROCm 7.x); loaded at start, extended
# (and re-written) if new shapes appear.  Set KA_TUNABLEOP=0 to use hipBLASLt's heuristics only.
DEFAULT_TUNABLEOP_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "tunableop_mi355x.csv")


ROUNDS = int(os.environ.get("KA_AUTOTUNE_ROUNDS", "3"))


def _time(fn, weights: List[torch.Tensor], reps: int = 12, rounds: int = 0) -> float:
    """us per call, the best of `rounds` timed runs of `reps` calls (rotating over the layers'
    weights so every call streams from HBM): candidates 1-2 us apart are otherwise ranked by noise."""
    for i in range(3):
        fn(weights[i % len(weights)])
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(max(1, rounds or ROUNDS)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(weights[i % len(weights)])
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


# ---- persisted plans ------------------------------------------------------------------------------
# The plan is a pure function of the hardware and the shapes (and of the consumer each projection
# feeds), so one tuned on an MI355X is committed (tuned/gemm_plan_mi355x.json) and loaded at engine
# start instead of re-timing every candidate: deterministic plans across boxes and runs.
# KA_GEMM_PLAN=file (default: use the file when it covers every shape, else tune) | tune | write
# (tune with KA_AUTOTUNE_ROUNDS rounds and merge the result into the file).
DEFAULT_PLAN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gemm_plan_mi355x.json")


def plan_key(M: int, N: int, K: int, ctx: str) -> str:
    return f"{M},{N},{K},{ctx}"


def _read_json(path: str) -> dict:
    """The plan file's contents, {} when it is missing or unreadable."""
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def load_plan(path: str, wanted: Dict[Tuple[int, int, int], str]) -> set:
    """Fill GEMM_PLAN from `path` for every wanted (M, N, K) -> consumer context it holds; returns
    the (M, N, K) still missing (to be tuned)."""
    plans = _read_json(path).get("plans", {})
    missing = set()
    for mnk, ctx in wanted.items():
        e = plans.get(plan_key(*mnk, ctx))
        if e is None:
            missing.add(mnk)
        else:
            GEMM_PLAN[mnk] = tuple(e[:3])
    logger.info("gemm plan: %d of %d entries from %s", len(wanted) - len(missing), len(wanted), path)
    return missing


def save_plan(path: str, report: Dict, ctx_of: Dict[Tuple[int, int], str]) -> None:
    data = _read_json(path)
    plans = data.setdefault("plans", {})
    for (M, N, K), r in report.items():
        plans[plan_key(M, N, K, ctx_of[(N, K)])] = [r["choice"], r["split"], r["cfg"], r["us"], r["blas_us"],
                                                   r.get("hand_us", r["us"])]
    repair_ladder(plans)
    data["device"] = torch.cuda.get_device_name() if torch.cuda.is_available() else "cpu"
    data["note"] = ("ops/autotune.py: [choice, split, cfg, us, hipBLASLt us, best hand-written us] "
                    "per M,N,K,consumer")
    with open(path, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)


def load_section(path: str, section: str) -> Dict[str, list]:
    """Entries of another persisted engine-start decision (`lm_head`, `decode_swiglu`, `prefill`) in the plan file."""
    return dict(_read_json(path).get(section, {}))


def save_section(path: str, section: str, entries: Dict[str, list]) -> None:
    data = _read_json(path)
    data.setdefault(section, {}).update(entries)
    with open(path, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)


def plan_mode() -> Tuple[str, str]:
    """(KA_GEMM_PLAN, plan file): `file` (load, tune what is missing), `tune` or `write`."""
    return os.environ.get("KA_GEMM_PLAN", "file"), os.environ.get("KA_GEMM_PLAN_FILE", DEFAULT_PLAN_FILE)


def _saved_section(section: str) -> Dict[str, list]:
    """The section's entries in `file` mode; nothing in `tune` / `write` mode, which re-time every key."""
    mode, path = plan_mode()
    return load_section(path, section) if mode == "file" else {}


def _write_section(section: str, entries: Dict[str, list]) -> None:
    mode, path = plan_mode()
    if mode == "write":
        save_section(path, section, entries)


# A hipBLASLt plan is kept only when it beats the best hand-written candidate by more than this
# fraction: within it the hand-written kernel is taken (no vendor kernel in the captured decode
# graphs, and one library's heuristics fewer between boxes).  KA_PLAN_BLAS_MARGIN=0: fastest wins.
# 0.15: every default decode bucket (HIPGRAPH_BUCKETS 1-256) is hand-written at 3 % already; the
# margin moves the optional buckets 160 / 320 / 384 off hipBLASLt for at most 15 % on one GEMM
# (profiles/r4/plan_big/: "hand_us" records the hand-written time next to hipBLASLt's).
BLAS_MARGIN = float(os.environ.get("KA_PLAN_BLAS_MARGIN", "0.15"))


def _hand_margin(M: int, N: int, K: int) -> float:
    """What a hand-written fused kernel may lose to a shape's unfused path: BLAS_MARGIN where the GEMM plan
    runs that shape on hipBLASLt (or holds no entry for it), nothing against a hand-written plan."""
    return BLAS_MARGIN if GEMM_PLAN.get((M, N, K), ("blas",))[0] == "blas" else 0.0


def _tunableop_begin() -> bool:
    """KA_TUNABLEOP=1: let torch TunableOp search hipBLASLt/rocBLAS solutions for the decode shapes
    while we time them (results cached in KA_TUNABLEOP_FILE); tuning is switched off afterwards so
    prefill's ragged shapes never trigger online tuning during serving."""
    if os.environ.get("KA_TUNABLEOP", "1") != "1":
        return False
    tun = torch.cuda.tunable
    tun.enable(True)
    fname = os.environ.get("KA_TUNABLEOP_FILE", DEFAULT_TUNABLEOP_FILE)
    if fname:
        tun.set_filename(fname)
        if os.path.exists(fname):
            tun.read_file(fname)
    tun.tuning_enable(True)
    tun.set_max_tuning_duration(int(os.environ.get("KA_TUNABLEOP_MS", "60")))
    # time candidates with operands rotated through a buffer larger than the 256 MB MALL, so the
    # choice reflects decode conditions (every layer's weights stream cold from HBM)
    tun.set_rotating_buffer_size(int(os.environ.get("KA_TUNABLEOP_ROTATING_MB", "1024")))
    return True


def _tunableop_end() -> None:
    """Stop tuning.  Results are written back only with KA_TUNABLEOP_WRITE=1 (to KA_TUNABLEOP_FILE):
    with one engine process per GPU, eight processes would otherwise rewrite the same file while
    others read it at start-up."""
    tun = torch.cuda.tunable
    tun.tuning_enable(False)
    if os.environ.get("KA_TUNABLEOP_WRITE", "0") == "1":
        try:
            tun.write_file()
        except Exception:  # pragma: no cover
            pass


@torch.inference_mode()
def tune_linear(groups: Dict[Tuple[int, int], List[torch.Tensor]], Ms: Sequence[int],
                norm_fed: Sequence[Tuple[int, int]] = (), bf16_partials: bool = True,
                consumers: Optional[Dict[Tuple[int, int], Tuple[Callable, bool]]] = None) -> Dict:
    """groups: (N, K) -> list of weight tensors of that shape (one per layer).
    norm_fed: shapes whose output goes straight into the fused residual + RMSNorm (o_proj and down
    at TP = 1).  Their candidates are timed together with that norm, split-K ones with the
    reduction deferred into it (as the model runs them), so a split plan is not charged for a
    reduce kernel the model never launches.
    consumers: (N, K) -> (fn(out, M), bf16) for other fused consumers — QKV -> the fused RoPE +
    KV-append + decode attention, which reduces split-K partials (bf16 ones when `bf16`) in its
    prologue: candidates are timed with that kernel, in the form the model runs them."""
    tunable = _tunableop_begin()
    try:
        return _tune(groups, Ms, set(norm_fed), bf16_partials, consumers or {})
    finally:
        if tunable:
            _tunableop_end()


# csrc/gemm_mfma.hip configurations timed for decode M (profiles/r2/autotune_*.txt: 128 x 64 rings
# win at M = 32-64, 128 x 128 at 96-256, 128 x 256 / 256 x 128 / 4-stage 128 x 128 at 192-256; the
# configurations that never won — one wave per SIMD, 32-deep rings, 64-row weight tiles, the 4-phase
# ping-pong — were removed: profiles/r2/gemm_sweep_v*.txt)
GM_TUNE_CFGS = (2, 3, 4, 5, 6, 8, 12, 19)


def gm_candidates(M: int, N: int, K: int, cfgs: Sequence[int] = ()):
    """(cfg, split) pairs of csrc/gemm_mfma.hip worth timing: tiles no taller than twice M and a
    grid of ~96-1024 workgroups on 256 CUs."""
    out = []
    if K % 64 or N % 16:   # rows past M re-read distinct rows r % M (never one clamped row: profiles/r5/gemm_big_clamp/)
        return out
    for cfg in cfgs or GM_TUNE_CFGS:
        bn, bm = gm_shape(cfg)
        if bm > 2 * M and bm > 64:
            continue
        tiles = ((N + bn - 1) // bn) * ((M + bm - 1) // bm)
        for split in (1, 2, 4, 8):
            if K % (64 * split) or K // split < 256:
                continue
            if split > 1 and tiles * split > 1024:
                continue
            if tiles * split < 96 and split < 8:
                continue
            out.append((cfg, split))
    return out


def _plan_runs(plan, M: int, K: int) -> bool:
    """A plan chosen for a larger bucket can run M rows (the row GEMV only up to its staged rows)."""
    return plan[0] != "rows" or rows_ok(M, K, plan[1])


def _run_plan(plan, x, w, fed: bool, bf16: bool):
    kind, split, cfg = plan
    if kind == "gm":
        return linear_gm(x, w, cfg, split, defer_reduce=fed, bf16_partials=bf16)
    if kind == "rows":
        return linear_rows(x, w, split, cfg, defer_reduce=fed)
    if kind == "big":
        return linear_big(x, w)
    return linear(x, w, split=split, defer_reduce=fed)   # skinny


def ladder_anomalies(plans: Dict[str, list], tol: float = 0.03) -> List[Tuple[str, str, float, float]]:
    """Persisted plan entries ({"M,N,K,ctx": [choice, split, cfg, us, ...]}) whose planned time exceeds
    the time planned for the next larger bucket of the same (N, K, consumer) by more than `tol`:
    [(key, larger key, us, larger us)].  The larger bucket's plan runs the smaller M too, so such an
    entry is a tuning miss (the ladder rule in _tune prevents it for new plans)."""
    by_shape: Dict[Tuple[int, int, str], List[Tuple[int, float, str]]] = {}
    for key, e in plans.items():
        m, n, k, ctx = key.split(",", 3)
        by_shape.setdefault((int(n), int(k), ctx), []).append((int(m), float(e[3]), key))
    out = []
    for rows in by_shape.values():
        rows.sort()
        for (m, us, key), (m2, us2, key2) in zip(rows, rows[1:]):
            if us > us2 * (1.0 + tol):
                out.append((key, key2, us, us2))
    return out


def repair_ladder(plans: Dict[str, list], tol: float = 0.03) -> List[str]:
    """Apply the ladder rule across runs: an entry tuned in an earlier run (another bucket subset, a
    PLAN_BUCKETS re-tune) whose time exceeds the next larger bucket's takes that bucket's plan (its
    kernels run the smaller M, in at most the larger bucket's time, which is recorded as an upper
    bound).  Largest bucket first, so a repaired plan can repair the next smaller one.  Returns the
    keys changed."""
    by_shape: Dict[Tuple[int, int, str], List[Tuple[int, str]]] = {}
    for key in plans:
        m, n, k, ctx = key.split(",", 3)
        by_shape.setdefault((int(n), int(k), ctx), []).append((int(m), key))
    changed = []
    for (n, k, ctx), rows in by_shape.items():
        rows.sort(reverse=True)
        for (m2, key2), (m, key) in zip(rows, rows[1:]):
            big, small = plans[key2], plans[key]
            plan = (big[0], big[1], big[2])
            if float(small[3]) > float(big[3]) * (1.0 + tol) and big[0] != "blas" and _plan_runs(plan, m, k):
                plans[key] = [big[0], big[1], big[2], float(big[3])] + list(small[4:])
                changed.append(key)
    return changed


def _tune(groups, Ms, norm_fed=frozenset(), bf16_partials: bool = True, consumers=None) -> Dict:
    report = {}
    consumers = consumers or {}
    for (N, K), ws in groups.items():
        ws = ws[: max(2, min(len(ws), 16))]
        cons = consumers.get((N, K))
        fed = (N, K) in norm_fed or cons is not None    # partials handed to a fused consumer
        bf16 = cons[1] if cons is not None else bf16_partials
        dev, dt = ws[0].device, ws[0].dtype
        g = torch.ones(N, device=dev, dtype=dt)
        # largest bucket first: each bucket also times the plan chosen for the next larger one (that
        # plan's kernels take any M up to its bucket), so a small bucket never keeps a plan slower
        # than the one a larger bucket runs (the ladder rule; B = 4 took 47.8 us for the Llama-3-8B
        # gate_up on the skinny kernel where B = 8's ring kernel took 42.2)
        larger = None
        for M in sorted(set(int(m) for m in Ms if m <= TILE_MAX_M), reverse=True):
            x = torch.randn(M, K, device=dev, dtype=dt)
            res = torch.zeros(M, N, device=dev, dtype=dt)
            if cons is not None:
                norm = (lambda h, M=M, fn=cons[0]: fn(h, M))
            elif fed:
                norm = (lambda h: rmsnorm(h, g, 1e-5, residual=res))
            else:
                norm = (lambda h: h)
            GEMM_PLAN.pop((M, N, K), None)
            t_blas = _time(lambda w: norm(torch.nn.functional.linear(x, w)), ws)
            best = ("blas", 0, 0, float("inf"))   # the best hand-written candidate
            if M <= SKINNY_MAX_M and K % 64 == 0 and N % 4 == 0:
                cands = sorted({skinny_split(M, N, K, t) for t in (256, 512, 1024, 2048)})
                for sp in cands:
                    t = _time(lambda w: norm(linear(x, w, split=sp, defer_reduce=fed)), ws)
                    if t < best[3]:
                        best = ("skinny", sp, 0, t)
            for sp in (1, 2, 4):   # row-streaming GEMV (M <= 4): split x rows per wave
                if not rows_ok(M, K, sp):
                    continue
                for rw in (1, 2, 4, 8):
                    t = _time(lambda w: norm(linear_rows(x, w, sp, rw, defer_reduce=fed)), ws)
                    if t < best[3]:
                        best = ("rows", sp, rw, t)
            for cfg, sp in gm_candidates(M, N, K):
                t = _time(lambda w: norm(linear_gm(x, w, cfg, sp, defer_reduce=fed, bf16_partials=bf16)), ws)
                if t < best[3]:
                    best = ("gm", sp, cfg, t)
            if M >= BIG_PLAN_MIN_M and big_gemm_ok(x, ws[0]):   # 256 x 256 tiles, one wave per SIMD
                t = _time(lambda w: norm(linear_big(x, w)), ws)
                if t < best[3]:
                    best = ("big", 0, 0, t)
            if larger is not None and larger[0] != "blas" and _plan_runs(larger, M, K):
                t = _time(lambda w: norm(_run_plan(larger, x, w, fed, bf16)), ws)
                if t < best[3]:
                    best = (larger[0], larger[1], larger[2], t)
            hand_us = best[3]   # the fastest hand-written candidate, reported whichever wins
            if best[3] > t_blas * (1.0 + BLAS_MARGIN):
                best = ("blas", 0, 0, t_blas)
            GEMM_PLAN[(M, N, K)] = (best[0], best[1], best[2])
            larger = GEMM_PLAN[(M, N, K)]
            report[(M, N, K)] = {"choice": best[0], "split": best[1], "cfg": best[2], "us": round(best[3], 1),
                                 "blas_us": round(t_blas, 1), "hand_us": round(hand_us, 1),
                                 "with": "attention" if cons is not None else "norm" if fed else None}
    logger.info("gemm plan: %s", report)
    return report


# ---- engine-start tuning (tune_engine); `model` is duck-typed: models/llama.py LlamaModel ------------


def _weights_by_shape(model, keys: Sequence[str]) -> Dict[Tuple[int, int], List[torch.Tensor]]:
    """(N, K) -> the layers' dense 2-D weights of that shape under `keys` (MoE expert stacks are 3-D)."""
    groups: Dict[Tuple[int, int], List[torch.Tensor]] = {}
    for L in model.layers:
        for k in keys:
            w = L.get(k)
            if w is not None and w.dim() == 2:
                groups.setdefault(tuple(w.shape), []).append(w)
    return groups


def tune_gemm_plan(model, buckets, attention_consumer=None) -> dict:
    """Pick hipBLASLt vs the hand-written decode GEMM per (bucket, N, K) on this model's weights.
    attention_consumer: ModelRunner._attention_consumer(), None where the caller's KV cache cannot feed it."""
    groups = _weights_by_shape(model, ("wqkv", "wo", "w13", "w2"))
    # O / down partials feed the norm directly at TP = 1, and in a TP rank's decode step when the collective
    # reduces them (models/llama.py `fuse` defers their split-K reduce into the norm): timed with that consumer
    local = getattr(model, "_local_comm", False) or getattr(model.comm, "splitk_norm", False)
    norm_fed = set(_weights_by_shape(model, ("wo", "w2"))) if local else set()
    lm = model.W["lm_head"]
    groups.setdefault(tuple(lm.shape), []).append(lm)
    consumers = {}
    if attention_consumer is not None and model.fuse_decode_rope and model.D == 128 and "wqkv" in model.layers[0]:
        # QKV is timed with its real consumer, the fused RoPE + KV append + decode attention
        # on a synthetic 128-token context (a norm stand-in picked a split plan whose partials
        # then slowed the attention prologue: profiles/phase_profile_c256_qkv_proxy_negative.txt)
        consumers[tuple(model.layers[0]["wqkv"].shape)] = (attention_consumer, model.bf16_qkv_partials)
    bf16 = getattr(model, "bf16_partials", False)
    ctx_of = {nk: ("attn" + ("-bf16" if consumers[nk][1] else "")) if nk in consumers else
              ("norm" + ("-bf16" if bf16 else "")) if nk in norm_fed else "plain" for nk in groups}
    wanted = {(M, N, K): ctx_of[(N, K)] for (N, K) in groups for M in set(buckets) if M <= TILE_MAX_M}
    mode, path = plan_mode()
    Ms = buckets
    if mode == "file":
        missing = load_plan(path, wanted)
        if not missing:
            return {"from": path}
        Ms = sorted({M for (M, _, _) in missing})
        groups = {nk: ws for nk, ws in groups.items() if any((M,) + nk in missing for M in Ms)}
    report = tune_linear(groups, Ms, norm_fed, bf16, consumers)
    if mode == "write":
        save_plan(path, report, ctx_of)
    return report


def _fused_min_m(fused: Dict[int, bool]) -> int:
    """Row counts no bucket timed: fused from the smallest bucket above which every timed bucket won."""
    return next((M for M in sorted(fused) if all(f for b, f in fused.items() if b >= M)), 1 << 30)


@torch.inference_mode()
def tune_lm_head(model, buckets, mask_bits) -> dict:
    """Per decode bucket: the fused LM head + masked argmax (csrc/gemm_big.hip) against the
    GEMM plan's LM head + masked_argmax, on the model's own LM head and a SAFE_DECODE mask row;
    fills ops.LM_HEAD_FUSED and the threshold for untimed row counts."""
    lm = model.W["lm_head"]
    if ops.LM_HEAD_MODE != "auto":
        return {}
    V, K = lm.shape
    report = {}
    key = lambda M: f"{M},{V},{K},{int(mask_bits is not None)}"   # noqa: E731
    saved = _saved_section("lm_head")   # persisted with the GEMM plan: the same decision on every box and run
    for M in sorted(set(buckets)):
        x = torch.randn(M, K, device=lm.device, dtype=lm.dtype)
        if not ops.lm_head_argmax_ok(x, lm, model.vocab_offset):
            return {}
        if key(M) in saved:
            fused, t_fu, t_un = saved[key(M)]
        else:
            midx = torch.zeros(M, dtype=torch.int32, device=lm.device) if mask_bits is not None else None
            t_un = _time(lambda w: ops.masked_argmax(ops.linear(x, w), mask_bits, midx, model.vocab_offset), [lm])
            t_fu = _time(lambda w: ops.lm_head_argmax(x, w, mask_bits, midx, model.vocab_offset), [lm])
            fused = t_fu < t_un * (1.0 + _hand_margin(M, V, K))
        ops.LM_HEAD_FUSED[M] = bool(fused)
        report[M] = {"fused_us": round(t_fu, 1), "unfused_us": round(t_un, 1), "fused": bool(fused)}
    _write_section("lm_head", {key(M): [r["fused"], r["fused_us"], r["unfused_us"]] for M, r in report.items()})
    ops.LM_HEAD_FUSED_MIN_M = _fused_min_m(ops.LM_HEAD_FUSED)
    logger.info("lm head plan: %s (fused from %d rows)", report, ops.LM_HEAD_FUSED_MIN_M)
    return report


@torch.inference_mode()
def tune_decode_swiglu(model, buckets) -> dict:
    """Per decode bucket: gate_up with the ring kernel's SwiGLU epilogue (ops.linear_gm_swiglu,
    each configuration) against the GEMM plan's gate_up + SiLU·mul, on the model's own w13
    rotated over layers; fills ops.DECODE_SWIGLU_CFG with the winners."""
    ops.DECODE_SWIGLU_CFG.clear()
    if ops.DECODE_SWIGLU == "0" or getattr(model.cfg, "is_moe", False):
        return {}
    ws = next(iter(_weights_by_shape(model, ("w13",)).values()), [])[:8]
    if not ws:
        return {}
    w2s = next(iter(_weights_by_shape(model, ("w2",)).values()), [])[:8]
    N, K = ws[0].shape
    report = {}
    key = lambda M: f"{M},{N},{K}"   # noqa: E731
    saved = _saved_section("decode_swiglu")   # persisted like the GEMM plan
    for M in sorted(set(buckets)):
        x = torch.randn(M, K, device=ws[0].device, dtype=ws[0].dtype)
        if not ops.decode_swiglu_ok(x, ws[0]):
            continue
        if key(M) in saved:
            cfg, t_fu, t_un = saved[key(M)]
            best = (int(cfg), t_fu if int(cfg) else t_un)
            fused = (int(cfg), t_fu)
        else:
            small = M <= ops.GEMV_SWIGLU_MAX_M and len(w2s) == len(ws)
            if small:
                # the unfused path at these rows computes SiLU·mul inside the down GEMV's staging
                # (ops.swiglu_linear): compare gate_up + down, both ways (indices pair w13 / w2)
                pair = {id(a): b for a, b in zip(ws, w2s)}
                t_un = _time(lambda w: ops.swiglu_linear(ops.linear(x, w, defer_reduce=True), pair[id(w)]), ws)
            else:
                t_un = _time(lambda w: ops.silu_mul(ops.linear(x, w, defer_reduce=True)), ws)
            fused = (0, float("inf"))
            cands = list(ops.DECODE_SWIGLU_CFGS)
            if M >= ops.BIG_PLAN_MIN_M and ops.swiglu_gemm_ok(x, ws[0]):
                cands.append(ops.DECODE_SWIGLU_BIG)   # csrc/gemm_big.hip's SwiGLU epilogue
            for cfg in cands:
                if small:
                    t = _time(lambda w: ops.linear(ops.linear_gm_swiglu(x, w, cfg), pair[id(w)]), ws)
                else:
                    t = _time(lambda w: ops.linear_gm_swiglu(x, w, cfg), ws)
                if t < fused[1]:
                    fused = (cfg, t)
            best = fused if fused[1] < t_un * (1.0 + _hand_margin(M, N, K)) else (0, t_un)
        ops.DECODE_SWIGLU_CFG[M] = best[0]   # 0 (unfused) is kept too: un-timed M take the next bucket
        # fused_us: the fastest SwiGLU-epilogue configuration's time, whether or not it was taken
        report[M] = {"cfg": best[0], "fused_us": round(fused[1], 1), "unfused_us": round(t_un, 1)}
    _write_section("decode_swiglu", {key(M): [r["cfg"], r["fused_us"], r["unfused_us"]] for M, r in report.items()})
    logger.info("decode swiglu plan: %s", report)
    return report


def _time_big_vs_blas(x, ws: List[torch.Tensor], reps: int = 6, rounds: int = 0) -> Tuple[float, float]:
    """(csrc/gemm_big.hip us, hipBLASLt us) of x @ w.T over the weights `ws`, hipBLASLt timed first."""
    t_blas = _time(lambda w: torch.nn.functional.linear(x, w), ws, reps=reps, rounds=rounds)
    return _time(lambda w: ops.linear_big(x, w), ws, reps=reps, rounds=rounds), t_blas


@torch.inference_mode()
def tune_prefill(model) -> dict:
    """Prefill / mixed-step projections (ops.PREFILL_GEMM auto): csrc/gemm_big.hip against hipBLASLt per (N, K)
    of the model's QKV / O / down at the row-count buckets of ops.PREFILL_BUCKETS, on the model's own weights
    rotated over layers (the persisted decision in the plan file, section prefill, unless KA_GEMM_PLAN=tune /
    write).  Fills ops.PREFILL_PLAN: gemm_big where it is within KA_PREFILL_MARGIN (default 0.02) of hipBLASLt."""
    ops.PREFILL_PLAN.clear()
    if ops.PREFILL_GEMM != "auto":
        return {}
    margin = float(os.environ.get("KA_PREFILL_MARGIN", "0.02"))
    saved = _saved_section("prefill")
    report = {}
    for (N, K), ws in _weights_by_shape(model, ("wqkv", "wo", "w2")).items():
        ws = ws[:4]
        for M in ops.PREFILL_BUCKETS:
            key = f"{M},{N},{K}"
            if key in saved:
                big, t_big, t_blas = saved[key]
            else:
                x = torch.randn(M, K, device=ws[0].device, dtype=ws[0].dtype)
                if not ops.big_gemm_ok(x, ws[0]):
                    break
                t_big, t_blas = _time_big_vs_blas(x, ws)
                big = t_big <= t_blas * (1.0 + margin)
                del x
            ops.PREFILL_PLAN[(M, N, K)] = bool(big)
            report[key] = [bool(big), round(float(t_big), 1), round(float(t_blas), 1)]
    _write_section("prefill", report)
    logger.info("prefill gemm plan: %s", report)
    return report


def tune_engine(model, buckets, mask_bits=None, attention_consumer=None) -> dict:
    """What an engine decides once from the loaded model's own weights, before it captures its decode graphs:
    the four reports by name, in the order run (the later three read GEMM_PLAN).  Off the GPU: nothing to tune."""
    if model.W["lm_head"].device.type != "cuda":
        return {"gemm": {}, "lm_head": {}, "decode_swiglu": {}, "prefill": {}}
    return {"gemm": tune_gemm_plan(model, buckets, attention_consumer),
            "lm_head": tune_lm_head(model, buckets, mask_bits),
            "decode_swiglu": tune_decode_swiglu(model, buckets),
            "prefill": tune_prefill(model)}
