"""The attention kernels of csrc/attention.hip against an fp64 reference, on probe inputs that turn a
lost, stale, doubled or misplaced token into an error of many ulps (tests/attention_probes.py; what
each probe catches is proven on the CPU by tests/test_attention_probes_cpu.py).

count and needle outputs are compared with `assert_exact_to_ulp` (one bf16 ulp); random and ramp
with `assert_attention_close` (at most 4 x the error of the bf16-emulating reference).

Measured kernel / emulated error ratios, the largest per (row, head) over all random and ramp cases
of this file on an MI355X (limit 4; the module prints them again at teardown, see them with -s):
    decode 4-wave   1.71   (kernel error at most 0.012 of the output's rms, emulated 0.012)
    decode 2-wave   1.87   (0.015, 0.016)
    fused           1.98   (0.013, 0.014)
    fused 2-wave    1.97   (0.015, 0.016)
    cascade         2.06   (0.015, 0.016)
    prefill         2.03   (0.018, 0.018)
The same comparator in tests/test_kernels_gpu.py, over its far more numerous (row, head) pairs,
measured at most 3.02 (test_decode_attention_rope_fused); no kernel exceeded 4, and no count or
needle case was off by more than one bf16 ulp.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU with -m "not gpu" deselected anyway
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import attention_probes as ap  # noqa: E402

DEV = "cuda"
RATIOS = {}


@pytest.fixture(autouse=True, scope="module")
def _lib():
    _hip.require()
    torch.manual_seed(0)
    yield
    for kernel, r in sorted(RATIOS.items()):
        print(f"\nlargest kernel/emulated error ratio, {kernel}: {r:.3f}")


def _check(kernel, case, got, want, q=None, k=None, v=None, what=""):
    """The family's comparator on the rows of non-empty sequences; padding rows must be zero."""
    rows = case.rows.to(got.device)
    if case.family in ("count", "needle"):
        ap.assert_exact_to_ulp(got[rows], want[rows], what)
    else:
        emu = case.reference(q, k, v, emulate=True)
        r = ap.assert_attention_close(got[rows], want[rows], emu[rows], f"{kernel} {what}")
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)
    pad = [r for s, c in enumerate(case.ctx_lens.tolist()) if c == 0
           for r in range(int(case.q_starts[s]), int(case.q_starts[s + 1]))]
    if pad and not case.shared:
        assert got[pad].abs().max().item() == 0, "padding row is not zero"


def _seed(*xs):
    return sum((i + 1) * 7919 * int(x) for i, x in enumerate(xs)) % (2 ** 31)


FAMILY_SEED = {"count": 1, "needle": 2, "random": 3, "ramp": 4}


def _two_wave_rows():
    """(S, row count check): S * hkv (hkv = 8) just past the 2-wave threshold of 4 x CUs workgroups."""
    if os.environ.get("KA_DECODE_NW2_MIN_WGS") is not None:
        pytest.skip("KA_DECODE_NW2_MIN_WGS is set: the 2-wave threshold is not the default")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    S = 4 * cus // 8 + 2
    assert S * 8 > 4 * cus
    return S


def _mixed_rows(family, S, ctxs, special):
    """S rows cycling through ctxs, `special` {row: ctx} on top; needle targets cycle per context."""
    seen, rows = {}, []
    for i in range(S):
        c = special.get(i, ctxs[i % len(ctxs)])
        t = None
        if family == "needle" and c > 0:
            ts = ap.needle_targets(c)
            t = ts[seen.get(c, 0) % len(ts)]
            seen[c] = seen.get(c, 0) + 1
        rows.append((c, t))
    return rows


# ------------------------------------------------------------------------------------------------
# ops.attention_decode


@pytest.mark.parametrize("width", ["wide", "tight"])
@pytest.mark.parametrize("family", ap.FAMILIES)
@pytest.mark.parametrize("hq,hkv", [(8, 2), (16, 1), (3, 1)])
def test_decode_four_waves(hq, hkv, family, width):
    """paged_decode_kernel<false, 4>: G = 4, 16 (every MFMA row a head) and 3; 2048 tokens are 16
    passes of the 4 waves; block table generous and exactly as wide as the longest row needs."""
    rows = ap.needle_rows(ap.DECODE_CTXS) if family == "needle" else list(ap.DECODE_CTXS)
    case = ap.decode_case(family, hq, hkv, rows, width, seed=_seed(hq, FAMILY_SEED[family])).to(DEV)
    got = ops.attention_decode(case.q, case.k_cache, case.v_cache, case.block_tables, case.ctx_lens, case.scale)
    _check("decode 4-wave", case, got, case.reference(), what=f"{family} hq={hq} hkv={hkv} {width}")


@pytest.mark.parametrize("family", ["count", "needle", "random"])
def test_decode_two_waves(family):
    """paged_decode_kernel<false, 2> (batch x hkv > 4 x CUs): chunks w, w + 2, ...; 63 / 64 / 65 sit
    on its pass boundary, the 700-token row walks 11 passes, one padding row."""
    S = _two_wave_rows()
    rows = _mixed_rows(family, S, ap.NW2_CTXS, {5: 0, 7: 700})
    case = ap.decode_case(family, 32, 8, rows, seed=FAMILY_SEED[family]).to(DEV)
    got = ops.attention_decode(case.q, case.k_cache, case.v_cache, case.block_tables, case.ctx_lens, case.scale)
    _check("decode 2-wave", case, got, case.reference(), what=family)


# ------------------------------------------------------------------------------------------------
# ops.decode_attention_rope


def _run_fused(case, shared=None):
    """-> (kernel output, rotated q, caches after) with the caches checked: bit-identical to
    ops.rope_kv_write's, and nothing but the rows' own slots written."""
    k0, v0 = case.k_cache.clone(), case.v_cache.clone()
    k1, v1 = case.k_cache.clone(), case.v_cache.clone()
    got = ops.decode_attention_rope(case.qkv_input(), case.positions, case.cos_sin, case.slots, k1, v1,
                                    case.block_tables, case.ctx_lens, case.hq, case.hkv, ap.D, case.scale,
                                    shared_blocks=shared)
    q, k2, v2 = case.rope_append(ops.rope_kv_write)
    assert torch.equal(k1, k2) and torch.equal(v1, v2), "caches differ from ops.rope_kv_write's"
    s = case.slots[case.slots >= 0].long()
    blk, off = s // ap.BS, s % ap.BS
    k0[blk, :, off, :] = k1[blk, :, off, :]
    v0[blk, :, :, off] = v1[blk, :, :, off]
    assert torch.equal(k0, k1) and torch.equal(v0, v1), "a cache slot other than the rows' own was written"
    return got, q, k1, v1


@pytest.mark.parametrize("split", [0, 6, -6])
@pytest.mark.parametrize("family", ["count", "needle", "random"])
@pytest.mark.parametrize("hq,hkv", [(8, 2), (28, 4), (15, 1), (3, 1)])
def test_fused_decode(hq, hkv, family, split):
    """paged_decode_kernel<true, 4> on bf16 qkv and on 6 split-K partials (fp32; -6: bf16): G = 4, 7,
    15 and 3; contexts including the new token, so 1 = the new token alone, 33 / 129 / 257 = one
    cached chunk, pass 1 full, pass 2 full; needles on the new token and the one before it."""
    ctxs = ap.FUSED_CTXS
    rows = (ap.needle_rows(ctxs) if family == "needle" else list(ctxs)) + [0]
    case = ap.fused_case(family, hq, hkv, rows, "tight" if split else "wide",
                         seed=_seed(hq, FAMILY_SEED[family], abs(split)), split=split).to(DEV)
    got, q, k, v = _run_fused(case)
    _check("fused", case, got, case.reference(q, k, v), q, k, v, what=f"{family} hq={hq} hkv={hkv} split={split}")


@pytest.mark.parametrize("family", ["count", "needle", "random"])
def test_fused_decode_two_waves(family):
    """paged_decode_kernel<true, 2>: (32, 8) at the 2-wave row count, contexts up to 200."""
    S = _two_wave_rows()
    rows = _mixed_rows(family, S, ap.NW2_CTXS, {5: 0})
    case = ap.fused_case(family, 32, 8, rows, seed=10 + FAMILY_SEED[family]).to(DEV)
    got, q, k, v = _run_fused(case)
    _check("fused 2-wave", case, got, case.reference(q, k, v), q, k, v, what=family)


@pytest.mark.parametrize("S", [5, 33])
@pytest.mark.parametrize("ns", ap.CASCADE_NS)
@pytest.mark.parametrize("family", ["count", "needle", "random"])
@pytest.mark.parametrize("hq,hkv", [(2, 2), (4, 2), (8, 2), (8, 1)])
def test_cascade(hq, hkv, family, ns, S):
    """Cascade (ns shared leading blocks attended by cascade_prefix_kernel<G>, G = 1, 2, 4, 8, and
    merged with each row's own part) == the plain fused kernel == fp64.  S rows with the padding
    row last: a partly filled last wave of 16 / G sequences.  Needles inside the prefix and in the
    own part.  The padding row returns the prefix attention and is not compared."""
    case = ap.fused_case(family, hq, hkv, ap.cascade_rows(family, ns, S), seed=_seed(hq, hkv, ns, S),
                         shared=ns).to(DEV)
    nsh = torch.tensor([ns], dtype=torch.int32, device=DEV)
    got, q, k, v = _run_fused(case, shared=nsh)
    plain, _, k2, v2 = _run_fused(case)
    assert torch.equal(k, k2) and torch.equal(v, v2)
    rows = case.rows.to(DEV)
    if family != "random":   # (random: both are held to the fp64 reference below)
        ap.assert_exact_to_ulp(got[rows], plain[rows].double(), f"cascade vs plain {family} ns={ns}")
    _check("cascade", case, got, case.reference(q, k, v), q, k, v, what=f"{family} hq={hq} hkv={hkv} ns={ns} S={S}")


# ------------------------------------------------------------------------------------------------
# ops.attention_prefill

_shape_id = ap.shape_id


@pytest.mark.parametrize("shape", ap.PREFILL_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("family", ap.FAMILIES)
@pytest.mark.parametrize("hq,hkv", [(8, 2), (4, 2), (8, 1), (2, 2)])
def test_prefill(hq, hkv, family, shape):
    """paged_prefill_kernel with 16, 32, 8 and 64 tokens per query tile: chunked prefill (5 rows
    behind 595 cached tokens), several tiles, a 1-row sequence, contexts one past and one short of
    a block.  count: every row is the running count up to its own position; needle: every row
    returns its own or the previous position, one row per sequence must not see the next one."""
    qlens, ctxs = shape
    case = ap.prefill_case(family, hq, hkv, qlens, ctxs, seed=_seed(hq, hkv, FAMILY_SEED[family])).to(DEV)
    got = ops.attention_prefill(case.q, case.k_cache, case.v_cache, case.block_tables, case.q_starts, case.ctx_lens,
                                max(qlens), case.scale)
    want = case.reference()
    if family == "count":
        assert (want.cpu() - ap.running_count(hq, hkv, qlens, ctxs)).abs().max().item() < 1e-12
    _check("prefill", case, got, want, what=f"{family} hq={hq} hkv={hkv} {_shape_id(shape)}")


@pytest.mark.parametrize("hq,hkv", [(8, 2), (2, 2)])
def test_prefill_out_leaves_other_rows_untouched(hq, hkv):
    """out= into a poisoned buffer, called for sequences 1.. only: sequence 0's rows keep the poison
    bit for bit, the others are the probe's answer."""
    qlens, ctxs = ap.PREFILL_SHAPES[1]
    case = ap.prefill_case("count", hq, hkv, qlens, ctxs, seed=5).to(DEV)
    out = torch.full_like(case.q, ap.POISON)
    ret = ops.attention_prefill(case.q, case.k_cache, case.v_cache, case.block_tables[1:], case.q_starts[1:],
                                case.ctx_lens[1:], max(qlens[1:]), case.scale, out=out)
    assert ret is out
    n0 = qlens[0]
    assert (out[:n0] == ap.POISON).all()
    ap.assert_exact_to_ulp(out[n0:], case.reference()[n0:], "prefill out=")
