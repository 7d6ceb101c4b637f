"""The GEMM probes of tests/gemm_probes.py can fail: a tiled fp32 reference GEMM passes them as it is
and is rejected with each of these breaks built in, at every (M, N, K, split) that
tests/test_gemm_probes_gpu.py runs on the kernels:

    mutation       rejected by
    drop_k         integer family, exact equality (bf16 output and sum of slabs)
    drop_step      the same
    double_step    the same
    stale_step     the same  (needs two k-steps in the last slice)
    swap_chunk     the same
    lose_slice     the same  (needs split-K)
    double_slice   the same  (needs split-K)
    row_shift      the same  (needs two rows: the kernels wrap a row index modulo M)
    gate/up swap   SwiGLU family, one bf16 ulp
    tie -> highest argmax family, exact index

Where the last output tile holds fewer than 8 elements (the row GEMV at N = 1, say) the shape is probed
with several input sets (gemm_probes.draw_seeds), and a mutation counts as rejected when one of them
rejects it: one output element alone hides two swapped k-chunks whenever the two sums agree.

The comparator the older tests use (atol 3e-2, rtol 2e-2 on randn x and randn * 0.02 w) lets drop_k
through where the lost product is small: at 2 of the 64 positions tried in the smallest shape of
test_gemm_mfma_all_configs, whose last tile is 8 x 16; the integer family rejects all 64
(test_old_comparator_passes_a_dropped_element).  Against an error of one element in one k position
the old comparison is a tolerance argument; these probes make it a plain fact.
"""
import pytest
import torch

from tests import gemm_probes as gp

CASES = gp.gemm_cases()


def _rejected(P, ref, bm, bn) -> bool:
    """Either way the GPU module reads a result: the bf16 output, or the sum of the slabs."""
    try:
        gp.assert_exact(P.sum(0).to(gp.BF), ref, "bf16 output", bm, bn)
        gp.assert_slabs_exact(P, ref, "slabs", bm, bn)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("kernel", ["gm", "big", "skinny", "rows"])
def test_integer_family_rejects_every_mutation(kernel):
    cases = [c for c in CASES if c[0] == kernel]
    assert cases
    applied = {m: 0 for m in gp.MUTATIONS}
    refs = {}                                             # (M, N, K, seed, slices): shared by the tile geometries
    for (_, M, N, K, slices, bm, bn) in cases:
        what = f"{kernel} M={M} N={N} K={K} slices={len(slices)} tile {bm}x{bn}"
        draws = []
        seeds = gp.draw_seeds(M, N, K, bm, bn)            # the input sets the GPU module uses
        # "any draw rejects" below stands only where the GPU module runs every draw: its gemm_skinny and
        # gemv_rows tests loop over draw_seeds; its ring and gemm_big tests run one input set and assert
        # that draw_seeds gives no more (their last tiles hold 16 elements or more)
        assert len(seeds) == 1 or kernel in ("skinny", "rows"), what
        for seed in seeds:
            x, w = gp.make_xw(M, N, K, seed)
            key = (M, N, K, seed, tuple(slices))
            if key not in refs:
                if len(refs) > 8:
                    refs.clear()
                slabs = gp.want_slabs(x, w, slices)       # every slab within the exactness condition
                ref = gp.want(x, w)
                assert torch.equal(slabs.sum(0), ref)
                refs[key] = (ref, gp.tiled_gemm(x, w, bm, bn, slices))
            ref, base = refs[key]
            base = gp.tiled_gemm(x, w, bm, bn, slices, base=base)    # this geometry's last tile, step by step
            assert not _rejected(base, ref, bm, bn), f"the unmutated reference fails: {what}"
            draws.append((x, w, ref, base))
        for mut in gp.MUTATIONS:
            if not gp.mutation_applies(mut, M, slices):
                continue
            applied[mut] += 1
            for kk in ((5, 37, 63) if mut == "drop_k" else (0,)):
                assert any(_rejected(gp.tiled_gemm(x, w, bm, bn, slices, mut, kk=kk, base=base), ref, bm, bn)
                           for (x, w, ref, base) in draws), f"{mut} (kk={kk}) passes the probe: {what}"
    assert all(applied.values()), applied
    print(f"\n{kernel}: {len(cases)} shapes; mutations rejected (shapes applied to): {applied}")


def test_failure_report_names_the_tile():
    M, N, K = 257, 272, 192
    x, w = gp.make_xw(M, N, K, 3)
    P = gp.tiled_gemm(x, w, 128, 128, gp.even_slices(K, 1), "drop_step")
    with pytest.raises(AssertionError) as e:
        gp.assert_exact(P.sum(0).to(gp.BF), gp.want(x, w), "case", 128, 128)
    msg = str(e.value)
    assert "m-tiles 2..2" in msg and "n-tiles 2..2" in msg and "(row, col, got, want)" in msg, msg


def test_exactness_condition_is_enforced():
    x = torch.ones(1, 512, dtype=gp.BF)
    with pytest.raises(ValueError):
        gp.want(x, x)                                   # 512 > 256
    with pytest.raises(ValueError):
        gp.want_swiglu(torch.ones(1, 64, dtype=gp.BF), torch.ones(32, 64, dtype=gp.BF))   # |g| = 64


def test_every_k_contributes_to_every_16_column_group():
    """What makes drop_k visible whatever k is: x has no zero and w has a non-zero in every (k, 16-row
    group), at the sparse densities too."""
    for (N, K) in [(8, 4096), (60, 448), (68, 4096), (16, 1792), (8192, 3584), (1, 512), (3, 2048)]:
        x, w = gp.make_xw(5, N, K, 11)
        assert bool((x != 0).all())
        for n0 in range(0, N, 16):
            assert bool((w[n0:n0 + 16] != 0).any(0).all()), (N, K, n0)


def test_round_bf16_is_one_rounding():
    v = torch.tensor([1.0, 1.00390625, 1.005859375, -3.0e-6, 255.5, 1.0 + 2 ** -8 + 2 ** -40], dtype=torch.float64)
    r = gp.round_bf16(v).double()
    assert r.tolist()[:3] == [1.0, 1.0, 1.0078125]            # a tie goes to even, above it rounds up
    assert float(r[5]) == 1.0078125                            # fp64 -> fp32 -> bf16 would give 1.0
    assert bool(((r - v).abs() <= v.abs() * 2 ** -8).all())


def _swiglu_shapes():
    out = []
    for cfg in gp.GM_ALL_CFGS:
        if gp.GM_TN[cfg] % 2 or cfg == 19:
            continue
        bn, bm = gp.GM_TILES[cfg]
        for nk in gp.GM_NKS:
            for M in gp.gm_rows(cfg):
                for I in (16, bn // 2 + 16):
                    out.append((M, I, 64 * nk, bm, bn // 2))
    for K in gp.BIG_KS:
        for M in gp.BIG_MS:
            for I in gp.BIG_SWIGLU_IS:
                out.append((M, I, K, 256, 128))
    return sorted(set(out))


def test_swiglu_family_rejects_a_gate_up_swap():
    one = tot = 0
    shapes = _swiglu_shapes()
    for (M, I, K, bm, bn) in shapes:
        x, w13 = gp.make_swiglu(M, I, K, gp.case_seed(M, I, K))
        ref = gp.want_swiglu(x, w13)
        g = x.float() @ w13[:I].float().t()
        u = x.float() @ w13[I:].float().t()
        a, b = gp.assert_swiglu(gp.swiglu_from_gu(g, u), ref, f"unmutated M={M} I={I} K={K}", bm, bn)
        one, tot = one + a, tot + b
        c0 = (I - 1) // 16 * 16                           # the last 16-column chunk
        g2, u2 = g.clone(), u.clone()
        g2[:, c0:c0 + 16], u2[:, c0:c0 + 16] = u[:, c0:c0 + 16], g[:, c0:c0 + 16]
        with pytest.raises(AssertionError):
            gp.assert_swiglu(gp.swiglu_from_gu(g2, u2), ref, "swapped", bm, bn)
    print(f"\nSwiGLU: {len(shapes)} shapes, fp32 epilogue one ulp from the fp64 reference in {one} of {tot} elements")


def test_argmax_family_rejects_the_higher_tie():
    for (V, K) in gp.ARGMAX_VK:
        for M in gp.ARGMAX_MS:
            x, w = gp.make_argmax_xw(M, V, K, gp.case_seed(M, V, K))
            logits = gp.want(x, w)
            for off in gp.ARGMAX_OFFS:
                midx = torch.tensor([0, 1, -1] * (M // 3 + 1), dtype=torch.int32)[:M]
                for masked in (False, True):
                    allowed = gp.allowed_tokens(gp.make_mask(V, off), midx, V, off) if masked else None
                    wi, wv = gp.expected_argmax(logits, allowed, off)
                    gp.assert_argmax(*gp.pick_argmax(logits, allowed, off), wi, wv, "lowest tie")
                    if allowed is not None:
                        assert bool(allowed.gather(1, (wi.long() - off)[:, None]).all())
                    with pytest.raises(AssertionError):
                        gp.assert_argmax(*gp.pick_argmax(logits, allowed, off, tie="highest"), wi, wv, "highest tie")


def test_old_comparator_passes_a_dropped_element():
    """The documented gap: randn x, randn * 0.02 w, atol 3e-2 / rtol 2e-2 (test_gemm_mfma_all_configs'
    comparator and smallest shape).  The last k-step of the last 128 x 128 tile loses one element: the
    old comparator passes wherever |x[m, k] w[n, k]| stays under its tolerance for the tile's rows and
    columns (the share is printed), the integer family rejects every position."""
    M, N, K, bm, bn = 8, 1040, 512, 128, 128
    g = torch.Generator()
    g.manual_seed(0)
    x = torch.randn(M, K, generator=g).to(gp.BF)
    w = (torch.randn(N, K, generator=g) * 0.02).to(gp.BF)
    ref = x.float() @ w.float().t()
    xi, wi = gp.make_xw(M, N, K, 0)
    refi = gp.want(xi, wi)
    sl = gp.even_slices(K, 1)
    passed = []
    for kk in range(64):
        got = gp.tiled_gemm(x, w, bm, bn, sl, "drop_k", kk=kk).sum(0).to(gp.BF)
        assert not torch.equal(got.float(), ref.to(gp.BF).float())           # the result did change
        try:
            torch.testing.assert_close(got.float(), ref, atol=3e-2, rtol=2e-2)
            passed.append(kk)
        except AssertionError:
            pass
        assert _rejected(gp.tiled_gemm(xi, wi, bm, bn, sl, "drop_k", kk=kk), refi, bm, bn)
    print(f"\nold comparator passes the dropped element at {len(passed)} of 64 positions; the integer family at 0")
    assert passed, "the old comparator caught every dropped element"
