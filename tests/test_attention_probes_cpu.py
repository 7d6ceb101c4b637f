"""Self-test of the attention probes (tests/attention_probes.py), on the CPU.

Two things are proven here, for every context length the GPU tests use:
  * a correct implementation (the fp32 `ops.reference`, through the same `ops` entry points the GPU
    tests call) passes each family's comparator, so a GPU failure is the kernel's;
  * every reference mutation - a lost, stale, doubled, zeroed or misplaced token, a dropped block,
    the wrong kv head, a causal mask off by one - is rejected by the count or the needle probe, so a
    kernel with that bug cannot pass.  There is no list of expected misses.
"""
import functools

import pytest
import torch

from ai_agent_kubectl_amd import ops
from tests import attention_probes as ap

HQ, HKV = 4, 2


def _compare(case, got, want, q=None, k=None, v=None, what=""):
    rows = case.rows
    if case.family in ("count", "needle"):
        ap.assert_exact_to_ulp(got[rows], want[rows], what)
    else:
        emu = case.reference(q, k, v, emulate=True)
        ap.assert_attention_close(got[rows], want[rows], emu[rows], what)


@pytest.mark.parametrize("family", ap.FAMILIES)
def test_reference_passes_decode_probes(family):
    ctxs = [c for c in ap.ALL_DECODE_CTXS if c in ap.DECODE_CTXS + ap.NW2_CTXS + (700,)] + [0]
    case = ap.decode_case(family, HQ, HKV, ap.needle_rows(ctxs) if family == "needle" else ctxs)
    got = ops.attention_decode(case.q, case.k_cache, case.v_cache, case.block_tables, case.ctx_lens, case.scale)
    _compare(case, got, case.reference(), what=f"decode {family}")
    pad = [r for r, c in enumerate(case.ctx_lens.tolist()) if c == 0]
    assert pad and got[pad].abs().max().item() == 0


@pytest.mark.parametrize("ns,split", [(0, 0), (0, 6), (0, -6)] + [(ns, 0) for ns in ap.CASCADE_NS])
@pytest.mark.parametrize("family", ["count", "needle", "random"])
def test_reference_passes_fused_probes(family, ns, split):
    if ns == 0:
        rows = (ap.needle_rows(ap.FUSED_CTXS) if family == "needle" else list(ap.FUSED_CTXS)) + [0]
    else:
        rows = ap.cascade_rows(family, ns, 12)
    case = ap.fused_case(family, HQ, HKV, rows, split=split, shared=ns, width="tight" if split else "wide")
    q, k2, v2 = case.rope_append()
    k1, v1 = case.k_cache.clone(), case.v_cache.clone()
    # (the CPU path has no split-K consumer: it gets the partials' sum in the kernels' order)
    got = ops.decode_attention_rope(case.qkv, case.positions, case.cos_sin, case.slots, k1, v1, case.block_tables,
                                    case.ctx_lens, HQ, HKV, ap.D, case.scale)
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    if split:
        assert case.partials.shape[0] == abs(split) and case.partials.dtype == (ap.BF if split < 0 else torch.float32)
    _compare(case, got, case.reference(q, k2, v2), q, k2, v2, what=f"fused {family} ns={ns}")
    # the poison survives where no token was appended, and every appended slot was overwritten
    assert (k2 == ap.POISON).any() and (k2[0] == ap.POISON).all() and (v2[0] == ap.POISON).all()
    for s, c in enumerate(case.ctx_lens.tolist()):
        if c:
            K, V = ap.gather_tokens(k2, v2, case.block_tables[s], c)
            assert K.abs().max().item() < 100 and V.abs().max().item() < 100


@pytest.mark.parametrize("shape", ap.PREFILL_SHAPES, ids=ap.shape_id)
@pytest.mark.parametrize("family", ap.FAMILIES)
def test_reference_passes_prefill_probes(family, shape):
    qlens, ctxs = shape
    case = ap.prefill_case(family, HQ, HKV, qlens, ctxs)
    got = ops.attention_prefill(case.q, case.k_cache, case.v_cache, case.block_tables, case.q_starts, case.ctx_lens,
                                max(qlens), case.scale)
    want = case.reference()
    _compare(case, got, want, what=f"prefill {family}")
    if family == "count":   # the fp64 reference itself against the answer known from the codes alone
        assert (want - ap.running_count(HQ, HKV, qlens, ctxs)).abs().max().item() < 1e-12


def test_count_decode_reference_is_the_known_count():
    ctxs = list(ap.ALL_DECODE_CTXS)
    case = ap.decode_case("count", HQ, HKV, ctxs)
    assert (case.reference() - ap.running_count(HQ, HKV, [1] * len(ctxs), ctxs)).abs().max().item() < 1e-12


def test_emulated_reference_error_is_bf16_sized():
    """The bf16-emulating reference differs from fp64 by bf16-rounding-sized amounts: more than
    nothing, and below 2^-5 of the output's rms (P and the output are each rounded to 8 bits)."""
    case = ap.decode_case("random", HQ, HKV, [129, 700, 2048])
    err = ap.normalised_error(case.reference(emulate=True), case.reference())
    print("emulated normalised error per row:", err.amax(dim=1).tolist())
    assert 1e-3 < err.min().item() and err.max().item() < 2.0 ** -5


@functools.lru_cache(maxsize=None)
def _decode_probes(ctx: int):
    out = []
    for family, rows in (("count", [ctx]), ("needle", ap.needle_rows([ctx]))):
        case = ap.decode_case(family, HQ, HKV, rows, seed=ctx)
        out.append((case, case.reference()))
    return out


@pytest.mark.parametrize("mutation,ctx", [pytest.param(m, c, id=f"{m.name}-{c}") for m in ap.DECODE_MUTATIONS
                                          for c in ap.ALL_DECODE_CTXS if m.defined(c, HKV)])
def test_decode_mutation_is_rejected(mutation, ctx):
    caught = []
    for case, want in _decode_probes(ctx):
        mutant = case.reference(mutation=mutation.fn).to(ap.BF)      # what a kernel with the bug returns
        assert ap.rejects(ap.assert_exact_to_ulp, want.to(ap.BF), want) is False
        if ap.rejects(ap.assert_exact_to_ulp, mutant, want):
            caught.append(case.family)
    print(f"{mutation.name} at {ctx} tokens: rejected by {caught}")
    assert caught, f"{mutation.name} at {ctx} tokens passes both the count and the needle probe"


@functools.lru_cache(maxsize=None)
def _prefill_probes(shape):
    out = []
    for family in ("count", "needle"):
        case = ap.prefill_case(family, HQ, HKV, *shape)
        out.append((case, case.reference()))
    return out


@pytest.mark.parametrize("shape", ap.PREFILL_SHAPES, ids=ap.shape_id)
@pytest.mark.parametrize("mutation", ap.PREFILL_MUTATIONS, ids=lambda m: m.name)
def test_prefill_mutation_is_rejected(mutation, shape):
    caught = []
    for case, want in _prefill_probes(shape):
        mutant = case.reference(mutation=mutation.fn).to(ap.BF)
        if ap.rejects(ap.assert_exact_to_ulp, mutant, want):
            caught.append(case.family)
    print(f"{mutation.name} at {shape}: rejected by {caught}")
    assert caught, f"{mutation.name} at {shape} passes both the count and the needle probe"


def test_needle_with_leaked_future_token_is_not_its_target():
    """The prefill needle row that also carries the needle of position + 1: with the mask one too
    wide its output is a mix of V[p] and V[p + 1], far from either."""
    case, want = _prefill_probes(ap.PREFILL_SHAPES[2])[1]
    mutant = case.reference(mutation=ap.PREFILL_MUTATIONS[1].fn)
    r = 65 // 2
    assert (mutant[r] - want[r]).abs().max().item() > 0.1
