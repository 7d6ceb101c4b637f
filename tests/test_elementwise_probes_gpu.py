"""The probes of tests/elementwise_probes.py against csrc/elementwise.hip, csrc/sampling.hip and the routing
kernels of csrc/moe.hip: the same cases tests/test_elementwise_probes_cpu.py proves sensitive, through
`ops.*` (align, sort and combine through the ka_* entry points, called the way ops.moe_experts calls them).
Outputs are written into sentinel frames wherever the op takes `out=`.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from ai_agent_kubectl_amd.ops._hip import check  # noqa: E402
from tests import elementwise_probes as ep  # noqa: E402

DEV = "cuda"
BF = ep.BF
_p, _st = ops._p, ops._stream


@pytest.fixture(autouse=True, scope="module")
def _lib():
    _hip.require()


def _id(v):
    if isinstance(v, dict):
        return "-".join(f"{k}{int(x)}" for k, x in v.items() if x or k in ("T",))
    return None


# ---- RoPE + KV append ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ep.rope_cases(), ids=_id)
def test_rope_kv_append(case):
    c = ep.rope_inputs(case)
    T, hq, hkv, d = c["T"], c["hq"], c["hkv"], c["d"]
    whole, view = ep.framed(T, hq * d, DEV)
    kc, vc = ep.rope_caches(c, DEV)
    qkv = ops.SplitK(c["P"].to(DEV), c["split"]) if c["P"] is not None else c["x"].to(DEV)
    q = ops.rope_kv_write(qkv, c["pos"].to(DEV), c["table"].to(DEV), c["slots"].to(DEV), kc, vc, hq, hkv, d,
                          q_out=view.view(T, hq, d))
    ep.assert_frame(whole, str(case))
    ep.assert_rope(c, q, kc, vc, ep.rope_want(c), str(case))
    if c["all_pad"]:
        assert bool((kc == ep.SENT).all()) and bool((vc == ep.SENT).all())


# ---- RMSNorm ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,hidden,split,p_bf16", ep.rms_cases())
def test_rmsnorm(rows, hidden, split, p_bf16):
    c = ep.rms_inputs(rows, hidden, split, p_bf16)
    what = f"rows={c['rows']} hidden={hidden} split={split} p_bf16={p_bf16} variant={c['variant']}"
    w = c["w"].to(DEV)
    P = c["P"].to(DEV) if split else None
    for with_res in (False, True):
        x = (c["x"] if split or not with_res else ep.rms_x_for_residual(c)).to(DEV)
        res = c["res"].to(DEV) if with_res else None
        want, wres = ep.rms_want(x, w, res)
        whole, view = ep.framed(c["rows"], hidden, DEV)
        r = res.clone() if with_res else None
        out = ops.rmsnorm(ops.SplitK(P, split) if split else x, w, ep.EPS, residual=r, out=view)
        ep.assert_frame(whole, what)
        if with_res:
            ep.assert_equal(r, wres, f"{what}: residual")
        ep.assert_rel(out, want, 2.0 ** -8, f"{what}: residual={with_res}")
        far = int(((out.double() - want).abs() > 0.5 * ep.bf16_ulp(want)).sum())
        print(f"\n{what} residual={with_res}: {far} of {out.numel()} outputs are the farther bf16 neighbour")


def test_rmsnorm_refuses_hidden_8200():
    x = torch.ones(2, 8200, device=DEV, dtype=BF)
    w = torch.ones(8200, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError):
        ops.rmsnorm(x, w, ep.EPS)
    with pytest.raises(RuntimeError):
        ops.rmsnorm(ops.SplitK(torch.ones(2, 2, 8200, device=DEV), 2), w, ep.EPS)


# ---- SiLU * mul, embedding -------------------------------------------------------------------------
def _silu(gu_or_splitk, T, I):
    whole, view = ep.framed(T, I, DEV)
    out = ops.silu_mul(gu_or_splitk, out=view)
    ep.assert_frame(whole, "silu_mul")
    return out


def test_silu_mul_every_bf16_gate():
    gu = ep.silu_exhaustive().to(DEV)
    want = ep.silu_want(gu)
    out = _silu(gu, 3, 65536)
    ep.assert_silu(out, want, "exhaustive gate")
    off = int(((out.double() - want).abs() > 0.5 * ep.bf16_ulp(want) + ep.SILU_FLOOR).sum())
    print(f"\nSiLU exhaustive: {off} of {out.numel()} outputs are the farther bf16 neighbour of the fp64 answer")


def test_silu_mul_grid_stride():
    T, I = ep.SILU_GRID
    gu = ep.silu_grid_input(DEV)
    assert T * I // 8 > ep.SILU_GRID_CAP
    ep.assert_silu(_silu(gu, T, I), ep.silu_want(gu), "grid-stride")


@pytest.mark.parametrize("split", ep.SILU_SPLITS)
def test_silu_mul_splitk(split):
    P, S = ep.silu_split_input(split)
    T, I = S.shape[0], S.shape[1] // 2
    ep.assert_silu(_silu(ops.SplitK(P.to(DEV), split), T, I), ep.silu_want(S), f"split {split}")


@pytest.mark.parametrize("off", ep.EMB_OFFSETS)
@pytest.mark.parametrize("hidden", ep.EMB_HIDDENS)
def test_embedding(hidden, off):
    table, ids = ep.emb_inputs(hidden, off)
    whole, view = ep.framed(ids.shape[0], hidden, DEV)
    out = ops.embedding(ids.to(DEV), table.to(DEV), vocab_offset=off, out=view)
    ep.assert_frame(whole, "embedding")
    ep.assert_equal(out, ep.emb_want(table, ids, off), f"embedding hidden={hidden} off={off}")


# ---- masked argmax ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,off", ep.argmax_cases())
def test_masked_argmax(B, V, off):
    c = ep.argmax_inputs(B, V, off)
    assert _hip.require().ka_argmax_slices(B, V) == c["slices"]
    wi, wv = ep.argmax_pick(c)
    logits, bits, midx = c["logits"].to(DEV), c["bits"].to(DEV), c["midx"].to(DEV)
    if B > 1:
        idx, val = ops.masked_argmax(logits, bits, midx, vocab_offset=off)
    else:                                                  # one call per probe row, each with its own mask row
        n = logits.shape[0]
        idx = torch.empty(n, dtype=torch.int32, device=DEV)
        val = torch.empty(n, dtype=torch.float32, device=DEV)
        one = (midx >= 0).int() - 1                        # 0: mask row 0 of the slice passed; -1: unmasked
        for r in range(n):
            ops.masked_argmax(logits[r:r + 1], bits[r:r + 1], one[r:r + 1], vocab_offset=off,
                              out_idx=idx[r:r + 1], out_val=val[r:r + 1])
    ep.assert_argmax(idx, val, wi, wv, f"B={B} V={V} off={off} slices={c['slices']}")


# ---- router top-k ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T,E,k", ep.topk_cases())
def test_moe_topk_pairs(T, E, k):
    lg = ep.topk_logits(T, E, k)
    w, ids = ops.moe_topk(lg.to(DEV), k)
    ep.assert_topk(w, ids, *ep.topk_want(lg, k), f"T={T} E={E} k={k}")


# ---- MoE align / sort / combine --------------------------------------------------------------------
def _align(ids_dev, R, e0, el):
    lib = _hip.require()
    counts = torch.full((el,), -1, dtype=torch.int32, device=DEV)
    lists = torch.full((el, R), -1, dtype=torch.int32, device=DEV)
    check(lib.ka_moe_align(_p(counts), _p(lists), _p(ids_dev), R, e0, el, _st()), "moe_align")
    return counts, lists


@pytest.mark.parametrize("R", sorted(ep.MOE_ROUTINGS))
def test_moe_align(R):
    T, k, cs = ep.MOE_ROUTINGS[R]
    ids = ep.moe_routing(R)
    for (e0, el) in ep.moe_windows(len(cs), cs):
        counts, lists = _align(ids.to(DEV), R, e0, el)
        ep.assert_align(counts, lists, ids, e0, el, f"R={R} e0={e0} el={el}")


@pytest.mark.parametrize("H", [8, 512])
@pytest.mark.parametrize("src_div", [1, 2])
@pytest.mark.parametrize("R", sorted(ep.MOE_ROUTINGS))
def test_moe_sort(R, src_div, H):
    lib = _hip.require()
    T, k, cs = ep.MOE_ROUTINGS[R]
    ids = ep.moe_routing(R)
    for (e0, el) in ep.moe_windows(len(cs), cs):
        what = f"R={R} src_div={src_div} H={H} e0={e0} el={el}"
        counts, lists = ep.moe_sort_lists(ids, e0, el)
        x = torch.randint(1, 100, (R // src_div + 1, H), generator=ep._gen(R + H)).to(BF)
        chunks = (R + 255) // 256 + el
        xs = torch.full((R, H), ep.SENT, dtype=BF, device=DEV)
        slot = torch.full((R,), -1, dtype=torch.int32, device=DEV)
        tab = torch.full((chunks * 4,), -1, dtype=torch.int32, device=DEV)       # stale entries must be zeroed
        xd, cd, ld = x.to(DEV), counts.to(DEV), lists.to(DEV)
        check(lib.ka_moe_sort(_p(xs), _p(slot), _p(tab), _p(xd), _p(cd), _p(ld), R, src_div, H, el, chunks, _st()),
              "moe_sort")
        ep.assert_sort(xs, slot, tab, ep.moe_sort_want(x, counts, lists, src_div, chunks), what)
        # and on the kernel's own lists: a permutation of the listed rows, grouped by expert in expert order
        kc, kl = _align(ids.to(DEV), R, e0, el)
        check(lib.ka_moe_sort(_p(xs), _p(slot), _p(tab), _p(xd), _p(kc), _p(kl), R, src_div, H, el, chunks, _st()),
              "moe_sort")
        ep.assert_sort(xs, slot, tab, ep.moe_sort_want(x, kc.cpu(), kl.cpu(), src_div, chunks), what + " (aligned)")


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("H", [8, 2048, 2056])
def test_moe_combine_exact(H, k):
    lib = _hip.require()
    T = 7
    for split in (0,) + ep.MOE_COMBINE_SPLITS:
        Y, P, w, ids = ep.moe_combine_inputs(T, k, H, split=split)
        for (e0, el) in ((0, 8), (2, 4), (8, 2)):
            what = f"combine H={H} k={k} split={split} e0={e0} el={el}"
            want = ep.moe_combine_want(Y, P, w, ids, e0, el)
            whole, out = ep.framed(T, H, DEV)
            Yd = ep.moe_poison_nonlocal(Y, ids, e0, el).to(DEV)
            Pd = ep.moe_poison_nonlocal(P, ids, e0, el).to(DEV) if split else None
            wd, idd = w.to(DEV), ids.to(DEV)
            check(lib.ka_moe_combine(_p(out), None if split else _p(Yd), _p(Pd), max(split, 1), _p(wd), _p(idd),
                                     T, k, H, e0, el, _st()), "moe_combine")
            ep.assert_frame(whole, what)
            ep.assert_equal(out, want.to(BF), what)
            if e0 == 8:
                assert not bool(out.any()), what


@pytest.mark.parametrize("fn", ["experts", "grouped-big", "grouped-gm"])
@pytest.mark.parametrize("R", [256, 1026])
def test_moe_block_on_hand_made_routing(R, fn, monkeypatch):
    """The whole block on routing the test wrote (not ops.moe_topk's), against the dense fp32 reference."""
    if fn != "experts":
        monkeypatch.setattr(ops, "MOE_PREFILL", fn.split("-")[1])
    T, k, cs = ep.MOE_ROUTINGS[R]
    E, H, I = len(cs), 512, 384
    g = ep._gen(R)
    x = torch.randn(T, H, generator=g).to(BF).to(DEV)
    tid = ep.moe_routing(R).to(DEV)
    tw = torch.rand(T, k, generator=g) + 0.25
    tw = (tw / tw.sum(1, keepdim=True)).to(DEV)
    for (e0, el) in ep.moe_windows(E, cs):
        w13 = (torch.randn(el, 2 * I, H, generator=g) * 0.05).to(BF).to(DEV)
        w2 = (torch.randn(el, H, I, generator=g) * 0.05).to(BF).to(DEV)
        f = ops.moe_experts if fn == "experts" else ops.moe_experts_grouped
        got = f(x, w13, w2, tw, tid, e0)
        want = ep.moe_dense_ref(x, w13, w2, tw, tid, e0)
        torch.testing.assert_close(got.float(), want, atol=5e-2, rtol=5e-2)
        if int(ep.moe_lists_want(tid.cpu(), e0, el)[0].sum()) == 0:
            assert not bool(got.any())
