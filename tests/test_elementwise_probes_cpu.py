"""The probes of tests/elementwise_probes.py can fail: at every case tests/test_elementwise_probes_gpu.py
runs, a torch emulation of the kernel passes the probe as it is and is rejected with each of these
breaks built in (each test asserts that every mutation was applied at least once):

    RoPE + KV append   table row pos + 1 for pairs >= 32, cos/sin swapped, sine sign flipped, second float4
                       group reused, K to the neighbouring token's slot, V token/dim exchanged in the block,
                       a padding token written, the clamped token of a partial window written, slice
                       dropped, slice doubled
    RMSNorm            one thread's vector lost, one wave's partial lost, mean over the padded length, eps
                       dropped, residual written back unrounded (truncated, and the norm fed the unrounded
                       sum), slice dropped, slice doubled
    SiLU * mul         gate/up swapped, sigmoid for SiLU, output x 1.015, second grid pass skipped, slice
                       dropped, slice doubled
    embedding          vocab offset ignored, last table row refused, columns past 2048 not written
    masked argmax      mask bit shifted by one, mask indexed by the local id, tie to the highest id, last
                       vector of a slice skipped
    router top-k       weights swapped between slots, tie to the higher id, renormalisation dropped, the
                       last expert ignored
    MoE routing        row dropped from a list, row listed under two experts, chunk start off by the earlier
                       experts' tails, stale table entries, combine skipping j = k - 1, combine including a
                       non-local expert, slice dropped, slice doubled

The last four tests keep on record what the older comparators of tests/test_kernels_gpu.py let through,
with those tests' shapes and seeds.
"""
import pytest
import torch

from tests import elementwise_probes as ep

BF = ep.BF


def _fails(fn, *a) -> bool:
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


# ---- RoPE ------------------------------------------------------------------------------------------
def test_rope_table_properties():
    for d in (64, 128):
        t = ep.rope_exact_table(d)
        half = d // 2
        cos, sin = t[:, :half], t[:, half:]
        assert bool((t * 4 == (t * 4).round()).all()) and float(t.abs().max()) <= 2
        assert bool((t[1:] != t[:-1]).all()) and bool((t[0] != t[-1]).all())      # neighbours differ in every pair
        assert bool((cos != sin).all())
        i = torch.arange(half)
        lo = i[i % 8 < 4]
        assert bool((cos[:, lo] != cos[:, lo + 4]).all()) and bool((sin[:, lo] != sin[:, lo + 4]).all())


def test_rope_probes_reject_every_mutation():
    cases = ep.rope_cases()
    applied = {m: 0 for m in ep.ROPE_MUTATIONS}
    kinds = set()
    for case in cases:
        c = ep.rope_inputs(case)
        what = str(case)
        kinds.add((ep.rope_is_window(c["T"], c["d"], c["bs"]), c["split"] > 0))
        pos = c["pos"].tolist()
        assert c["table"].shape[0] - 1 in pos and (0 in pos or c["T"] == 1)
        want = ep.rope_want(c)
        if not c["real"]:
            for t in want[:3]:
                assert torch.equal(t.to(BF).double(), t), what        # the exact family is exact in bf16
        if c["P"] is not None:
            assert torch.equal(c["P"].sum(0).to(BF), c["x"])
        ep.assert_rope(c, *ep.rope_emulate(c), want, what)
        if c["all_pad"]:
            k0, v0 = ep.rope_caches(c)
            assert torch.equal(want[1].to(BF), k0) and torch.equal(want[2].to(BF), v0)
        if c["real"]:
            continue
        for mut in ep.ROPE_MUTATIONS:
            if not ep.rope_mutation_applies(mut, c):
                continue
            applied[mut] += 1
            assert _fails(ep.assert_rope, c, *ep.rope_emulate(c, mut), want, what), f"{mut} passes: {what}"
    assert all(applied.values()), applied
    assert kinds == {(w, s) for w in (False, True) for s in (False, True)}
    print(f"\nRoPE: {len(cases)} cases; mutations rejected (cases applied to): {applied}")


def test_rope_slot_patterns_cover_the_listed_ones():
    seen = set()
    for case in ep.rope_cases():
        c = ep.rope_inputs(case)
        s, T, bs = c["slots"].tolist(), c["T"], c["bs"]
        v = [x for x in s if x >= 0]
        assert 0 not in v and len(set(v)) == len(v) and max(v, default=0) < c["NB"] * bs
        if not v:
            seen.add("all_pad")
        for w0 in range(0, T, 16):
            win = s[w0:w0 + 16]
            blocks = {x // bs for x in win if x >= 0}
            if all(x < 0 for x in win):
                seen.add("pad_window")
            elif len(win) < 16 and win[-1] < 0:
                seen.add("pad_last_partial")
            elif win[0] < 0:
                seen.add("pad_first")
            elif len(blocks) == 2 and max(blocks) - min(blocks) > 1:
                seen.add("straddle")
            elif win == sorted(win, reverse=True) and len(win) > 1:
                seen.add("desc")
            elif len(blocks) == 1:
                seen.add("inblock")
    assert seen == {"all_pad", "pad_window", "pad_last_partial", "pad_first", "straddle", "desc", "inblock"}, seen


# ---- RMSNorm ---------------------------------------------------------------------------------------
def test_rms_variants_and_probe_positions():
    got = {(r, h, s): ep.rms_variant(r, h, s) for r in (1, 1025) for h in ep.RMS_HIDDENS for s in (False, True)}
    assert got[(1, 2048, False)] == (256, 1, 4) and got[(1, 2056, False)] == (512, 1, 8)
    assert got[(1025, 4096, False)] == (256, 2, 4) and got[(1025, 2056, False)] == (256, 2, 4)
    assert got[(1, 4104, False)] == (256, 4, 2) and got[(1025, 8192, False)] == (256, 4, 2)
    assert got[(1025, 4096, True)] == (512, 1, 8) and got[(1, 8192, True)] == (512, 2, 4)
    assert got[(1025, 8192, True)] == (256, 4, 2) and got[(1025, 4104, True)] == (256, 4, 2)
    launched = {ep.rms_variant(r or 1, h, s > 0)[:2] + (s > 0,) for r, h, s, _ in ep.rms_cases()}
    assert launched == {(256, 1, False), (512, 1, False), (256, 2, False), (256, 4, False),
                        (256, 1, True), (512, 1, True), (512, 2, True), (256, 4, True)}
    p = ep.rms_probe_positions(8192, 256, 4)
    for q in (0, 7, 8, 2047, 2048, 4095, 4096, 6143, 6144, 8191):
        assert q in p
    for i in range(4):
        for w in range(4):
            assert any((q // 8) // 256 == i and ((q // 8) % 256) // 64 == w for q in p)


def test_rms_probes_reject_every_mutation():
    cases = ep.rms_cases()
    applied = {m: 0 for m in ep.RMS_MUTATIONS}
    for (rows, hidden, split, pb) in cases:
        c = ep.rms_inputs(rows, hidden, split, pb)
        what = f"rows={c['rows']} hidden={hidden} split={split} p_bf16={pb} variant={c['variant']}"
        assert c["rows"] > len(c["probes"]), what
        if split:
            assert torch.equal(c["P"].float().sum(0).to(BF), c["x"]) and c["P"].dtype == (BF if pb else torch.float32)
        for with_res in (False, True):
            x = c["x"] if split or not with_res else ep.rms_x_for_residual(c)
            res = c["res"] if with_res else None
            want, wres = ep.rms_want(x, c["w"], res)
            assert bool((want != 0).all()), what
            out, r = ep.rms_emulate(c, x, with_res)
            ep.assert_rel(out, want, 2.0 ** -8, what)
            if with_res:
                ep.assert_equal(r, wres, what + " residual")
                assert not torch.equal(wres.float(), x.float() + res.float())      # the add does round somewhere
            for mut in ep.RMS_MUTATIONS:
                if not ep.rms_mutation_applies(mut, c, with_res):
                    continue
                applied[mut] += 1
                out, r = ep.rms_emulate(c, x, with_res, mut)
                bad = _fails(ep.assert_rel, out, want, 2.0 ** -8, what)
                if with_res:
                    bad = bad or _fails(ep.assert_equal, r, wres, what)
                assert bad, f"{mut} passes: {what} residual={with_res}"
    assert all(applied.values()), applied
    print(f"\nRMSNorm: {len(cases)} cases x (plain, residual); mutations rejected (applied to): {applied}")


# ---- SiLU * mul, embedding -------------------------------------------------------------------------
def test_silu_bound_holds_for_the_fp32_formula_with_margin():
    """The documented margin: outside the overflow floor the fp32 formula is within 2^-16 (relative) of
    the fp64 value, under 1 % of a bf16 ulp, so its bf16 rounding stays inside the one-ulp bound."""
    gu = ep.silu_exhaustive()
    want = ep.silu_want(gu)
    f32 = ep.silu_emulate_fp32(gu).double()
    err = (f32 - want).abs()
    big = want.abs() > ep.BF16_MAX                                        # gate x up past the largest bf16
    assert 0 < int(big.sum()) < 256 and bool((f32[big].abs() > ep.BF16_MAX).all())
    assert bool((err <= ep.SILU_FP32_REL * want.abs() + ep.SILU_FLOOR)[~big].all())
    over = gu[:, :65536].float() < -88.7228                               # exp(-g) overflows fp32
    assert bool((f32[over] == 0).all()) and float(want[over].abs().max()) < ep.SILU_FLOOR / 1.9
    assert float(want[~over].abs().min()) == 0.0                          # the gate 0 patterns
    ep.assert_silu(f32.float().to(BF), want, "fp32 emulation")
    one = int(((f32.float().to(BF).double() - want).abs() > 0.5 * ep.bf16_ulp(want)).sum())
    print(f"\nSiLU exhaustive: 3 x 65536 gates, fp32 formula rounds to the farther bf16 neighbour in {one} elements")


def test_silu_probes_reject_every_mutation():
    applied = {m: 0 for m in ep.SILU_MUTATIONS}
    runs = [("exhaustive", ep.silu_exhaustive(), None), ("grid", ep.silu_grid_input(), None)]
    runs += [(f"split {s}", ep.silu_split_input(s)[1], ep.silu_split_input(s)[0]) for s in ep.SILU_SPLITS]
    assert runs[1][1].shape[0] * runs[1][1].shape[1] // 16 > ep.SILU_GRID_CAP
    for name, gu, P in runs:
        want = ep.silu_want(gu)
        ep.assert_silu(ep.silu_emulate(gu, None, P), want, name)
        for mut in ep.SILU_MUTATIONS:
            if mut.startswith("slice") and P is None:
                continue
            if mut == "second_pass_skipped" and name != "grid":
                continue
            applied[mut] += 1
            assert _fails(ep.assert_silu, ep.silu_emulate(gu, mut, P), want, name), f"{mut} passes: {name}"
    assert all(applied.values()), applied
    print(f"\nSiLU: {len(runs)} inputs; mutations rejected (applied to): {applied}")


def test_embedding_probes_reject_every_mutation():
    applied = {m: 0 for m in ep.EMB_MUTATIONS}
    for hidden in ep.EMB_HIDDENS:
        for off in ep.EMB_OFFSETS:
            table, ids = ep.emb_inputs(hidden, off)
            want = ep.emb_want(table, ids, off)
            assert bool((want[[0, 3, 4, 5, 8]] == 0).all()) and bool((want[[1, 2, 6, 7]] != 0).all())
            for mut in ep.EMB_MUTATIONS:
                got = ep.emb_want(table, ids, off, mut)
                if mut == "offset_ignored" and off == 0 or mut == "tail_skipped" and hidden <= 2048:
                    continue
                applied[mut] += 1
                assert not torch.equal(got, want), (mut, hidden, off)
    assert all(applied.values()), applied


# ---- masked argmax ---------------------------------------------------------------------------------
def test_argmax_probes_reject_every_mutation():
    applied = {m: 0 for m in ep.ARGMAX_MUTATIONS}
    sliced = set()
    cases = ep.argmax_cases()
    for (B, V, off) in cases:
        c = ep.argmax_inputs(B, V, off)
        what = f"B={B} V={V} off={off} slices={c['slices']}"
        sliced.add(c["slices"] > 1)
        wi, wv = ep.argmax_pick(c)
        for r, (kind, hot, masked) in enumerate(c["rows"]):                # the answer is the one the row was built for
            if kind == "probe":
                assert (int(wi[r]), float(wv[r])) == (hot[0] + off, 10.0), (what, r)
            elif kind == "all_masked":
                assert int(wi[r]) == off and float(wv[r]) == float("-inf"), (what, r)
            else:
                assert int(wi[r]) == min(h for h in hot if h not in masked) + off and float(wv[r]) == 10.0, (what, r)
        for mut in ep.ARGMAX_MUTATIONS:
            if mut == "mask_local" and off == 0:
                continue
            applied[mut] += 1
            assert _fails(ep.assert_argmax, *ep.argmax_pick(c, mut), wi, wv, what), f"{mut} passes: {what}"
    assert all(applied.values()) and sliced == {False, True}, (applied, sliced)
    assert ep.argmax_slices(1, 128256) == 16 and ep.argmax_slices(127, 128256) == 4 and ep.argmax_slices(128, 128256) == 1
    print(f"\nmasked argmax: {len(cases)} cases; mutations rejected (applied to): {applied}")


# ---- router top-k ----------------------------------------------------------------------------------
def test_topk_probes_reject_every_mutation():
    applied = {m: 0 for m in ep.TOPK_MUTATIONS}
    cases = ep.topk_cases()
    for (T, E, k) in cases:
        lg = ep.topk_logits(T, E, k)
        what = f"T={T} E={E} k={k}"
        ww, wi = ep.topk_want(lg, k)
        if T >= 2:                                                         # the all-equal row
            assert wi[1].tolist() == list(range(k)) and bool(((ww[1] - 1.0 / k).abs() < 1e-12).all())
        ep.assert_topk(*ep.topk_emulate(lg, k), ww, wi, what)
        for mut in ep.TOPK_MUTATIONS:
            if not ep.topk_mutation_applies(mut, T, E, k):
                continue
            applied[mut] += 1
            assert _fails(ep.assert_topk, *ep.topk_emulate(lg, k, mut), ww, wi, what), f"{mut} passes: {what}"
    assert all(applied.values()), applied
    print(f"\nrouter top-k: {len(cases)} cases; mutations rejected (applied to): {applied}")


# ---- MoE routing -----------------------------------------------------------------------------------
def test_moe_routing_covers_the_listed_counts():
    counts = [c for _, _, cs in ep.MOE_ROUTINGS.values() for c in cs]
    for c in (0, 1, 64, 65, 256, 257, 513):
        assert c in counts
    for R, (T, k, cs) in ep.MOE_ROUTINGS.items():
        ids = ep.moe_routing(R)
        assert ids.shape == (T, k) and torch.bincount(ids.flatten().long(), minlength=len(cs)).tolist() == list(cs)
        e0, el = ep.moe_windows(len(cs), cs)[-1]
        assert int(ep.moe_lists_want(ids, e0, el)[0].sum()) == 0           # the window without a local row
    assert sorted(ep.MOE_ROUTINGS) == [1, 255, 256, 257, 1026]


def test_moe_probes_reject_every_mutation():
    applied = {m: 0 for m in ep.MOE_MUTATIONS}
    for R, (T, k, cs) in ep.MOE_ROUTINGS.items():
        ids = ep.moe_routing(R)
        for (e0, el) in ep.moe_windows(len(cs), cs):
            what = f"R={R} e0={e0} el={el}"
            counts, lists = ep.moe_align_emulate(ids, e0, el)
            ep.assert_align(counts, lists, ids, e0, el, what)
            for mut in ("row_dropped", "row_twice"):
                mc, ml = ep.moe_align_emulate(ids, e0, el, mut)
                if torch.equal(mc, counts):
                    continue
                applied[mut] += 1
                assert _fails(ep.assert_align, mc, ml, ids, e0, el, what), f"{mut} passes: {what}"
            for src_div in (1, 2):
                for H in (8, 512):
                    x = torch.randint(1, 100, (R // src_div + 1, H), generator=ep._gen(R + H)).to(BF)
                    chunks = (R + 255) // 256 + el
                    want = ep.moe_sort_want(x, counts, lists, src_div, chunks)
                    assert bool((want[0][:int(counts.sum())] != ep.SENT).all())
                    for mut in ("chunk_start_tail", "stale_table"):
                        got = ep.moe_sort_want(x, counts, lists, src_div, chunks, mut)
                        if all(torch.equal(a, b) for a, b in zip(got, want)):
                            continue
                        applied[mut] += 1
                        assert _fails(ep.assert_sort, *got, want, what), f"{mut} passes: {what}"
    for H in (8, 2048, 2056):
        for k in (1, 2, 4):
            for split in (0,) + ep.MOE_COMBINE_SPLITS:
                Y, P, w, ids = ep.moe_combine_inputs(7, k, H, split=split)
                for (e0, el) in ((0, 8), (2, 4), (8, 2)):
                    what = f"combine H={H} k={k} split={split} e0={e0} el={el}"
                    want = ep.moe_combine_want(Y, P, w, ids, e0, el)
                    assert torch.equal(want.to(BF).double(), want) and float(want.abs().max()) <= 20, what
                    if e0 == 8:
                        assert not bool(want.any())
                    Yp = ep.moe_poison_nonlocal(Y, ids, e0, el)
                    Pp = ep.moe_poison_nonlocal(P, ids, e0, el) if P is not None else None
                    ep.assert_equal(ep.moe_combine_want(Yp, Pp, w, ids, e0, el).to(BF), want, what)
                    for mut in ("skip_last_j", "nonlocal_included", "slice_drop", "slice_double"):
                        if mut.startswith("slice") and (P is None or e0 == 8):
                            continue
                        got = ep.moe_combine_want(Yp, Pp, w, ids, e0, el, mut)
                        if torch.equal(got, want) and mut in ("skip_last_j", "nonlocal_included"):
                            continue                                      # no local last slot / no non-local slot here
                        applied[mut] += 1
                        assert _fails(ep.assert_equal, got.to(BF), want, what), f"{mut} passes: {what}"
    assert all(applied.values()), applied
    print(f"\nMoE routing: mutations rejected (applied to): {applied}")


# ---- what the older comparators let through --------------------------------------------------------
def _close(a, b, atol, rtol=0.02):
    torch.testing.assert_close(a.float(), b.float(), atol=atol, rtol=rtol)


def test_old_rope_comparator_passes_the_next_table_row():
    """test_rope_kv_write: randn qkv, the real table, positions below 4000, close(atol=2e-2).  Reading the
    cos/sin row of pos + 1 for every pair >= 32 stays under the tolerance; the exact family rejects it at
    every case (above)."""
    from ai_agent_kubectl_amd.ops import reference as ref
    torch.manual_seed(0)
    T, hq, hkv, d = 23, 32, 8, 128
    qkv = torch.randn(T, (hq + 2 * hkv) * d).to(BF)
    cs = ref.rope_cos_sin(4096, d, 5e5)
    pos = torch.randint(0, 4000, (T,), dtype=torch.int32)
    slots = torch.randperm(64 * 16)[:T].int()
    c = dict(T=T, hq=hq, hkv=hkv, d=d, bs=16, pos=pos, slots=slots, NB=64, table=cs, P=None, x=qkv)
    q, k, _ = ep.rope_emulate(c)
    qm, km, _ = ep.rope_emulate(c, "row_next_hi")
    assert not torch.equal(q, qm) and not torch.equal(k, km)
    _close(qm, q, atol=2e-2)
    _close(km, k, atol=2e-2)
    print(f"\nold RoPE comparator: max difference {float((qm.float() - q.float()).abs().max()):.4f} passes atol 2e-2")


@pytest.mark.parametrize("rows,hidden", [(37, 4096), (5, 8192)])
def test_old_rmsnorm_comparator_passes_lost_vectors(rows, hidden):
    """test_rmsnorm: randn x, close(atol=2e-2).  One thread's 16-byte vector missing from the sum of squares
    passes, and so do eight threads' vectors; only a whole wave's is caught."""
    from ai_agent_kubectl_amd.ops import reference as ref
    torch.manual_seed(0)
    x = torch.randn(rows, hidden).to(BF)
    w = (1 + 0.1 * torch.randn(hidden)).to(BF)
    want = ref.rmsnorm(x, w, 1e-5)

    def lossy(nvec_lost):
        xf = x.float()
        ss = xf.pow(2).sum(-1, keepdim=True) - xf[:, :8 * nvec_lost].pow(2).sum(-1, keepdim=True)
        return (xf * torch.rsqrt(ss / hidden + 1e-5) * w.float()).to(BF)
    for n in (1, 8):
        assert not torch.equal(lossy(n), want)
        _close(lossy(n), want, atol=2e-2)
    assert _fails(_close, lossy(64), want, 2e-2)


def test_old_silu_comparator_passes_a_scaled_output():
    """test_silu_mul_and_embedding: randn gu, close(atol=2e-2) with rtol 2e-2: every output x 1.015 passes."""
    from ai_agent_kubectl_amd.ops import reference as ref
    torch.manual_seed(0)
    gu = torch.randn(19, 2 * 14336).to(BF)
    _close(ep.silu_emulate(gu, "scaled"), ref.silu_mul(gu), atol=2e-2)
    assert _fails(ep.assert_silu, ep.silu_emulate(gu, "scaled"), ep.silu_want(gu), "scaled")


def test_old_topk_comparator_passes_swapped_weights():
    """test_moe_topk sorted ids and weights separately: the two weights of every token swapped pass."""
    from ai_agent_kubectl_amd.ops import reference as ref
    torch.manual_seed(0)
    lg = torch.randn(50, 8).to(BF)
    w1, i1 = ep.topk_emulate(lg, 2, "weights_swapped")
    w2, i2 = ref.moe_topk(lg, 2)
    assert torch.equal(i1.sort(1).values, i2.sort(1).values)
    _close(w1.sort(1).values, w2.sort(1).values, atol=1e-5)
    assert _fails(ep.assert_topk, w1, i1, *ep.topk_want(lg, 2), "swapped")
