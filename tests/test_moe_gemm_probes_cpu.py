"""The MoE GEMM probes of tests/moe_gemm_probes.py can fail: plain-torch emulators of moe_gemm_kernel<MT>
and of the grouped gemm256_kernel pass them as they are and are rejected with each of these breaks built
in, on every input set tests/test_moe_gemm_probes_gpu.py runs (it imports the same case lists):

    mutation          applies to                       rejected by
    drop_k, drop_step, swap_chunk   both                exact equality with the fp64 product / one bf16 ulp
    lose_slice, double_slice        moe_gemm, split > 1  exact equality of every slab
    wrong_expert      both (two experts / two tiles of one workgroup)   one weight seed per expert
    stale_rows        both (two row chunks / two chunks on one workgroup)   distinct random rows
    src_div_ignored   moe_gemm, src_div 2              distinct random rows
    short_slice_full  moe_gemm, K 320 / 2 and 448 / 3  exact slabs
    chunk_clamp       moe_gemm, one-chunk slices       exact slabs
    row_clamp         moe_gemm, a ragged row chunk     the decoy row's sentinel
    hole_consumed     grouped, unused entries          the sentinel of the gap at sorted rows 0 and 1
    skip_after_hole   grouped, persistent table        the lost tile's sentinel
    wrap_stored       grouped, gnr < 256 before a gap  the gap's sentinel
    sorted_not_slot   grouped, bf16                    the sentinel of the slot row never written
    gate_up_swap      grouped, SwiGLU                  one bf16 ulp

A break that cannot apply to a case is skipped by moe_target / grouped_applies, never silently; every
break applies to, and is rejected on, at least one case (asserted over the whole list).  The persistent
table is sized from the device on the GPU; here the proof runs it for 256 workgroups (the MI355X), and its
workgroup patterns are checked for 64, 104 and 304 too.
"""
import pytest
import torch

from tests import gemm_probes as gp
from tests import moe_gemm_probes as mp



def _rejected(check, *a) -> bool:
    try:
        check(*a)
    except AssertionError:
        return True
    return False


def test_moe_case_list_covers_what_the_issue_names():
    cases = mp.moe_cases()
    assert {c[0] for c in cases} == set(mp.MOE_MAX_ROWS) and {mp.moe_mt(c[0]) for c in cases} == {1, 2, 4, 8}
    assert {(c[2], c[3]) for c in cases} == set(mp.MOE_KS)
    assert mp.moe_slices(320, 2) == [(0, 192), (192, 320)] and mp.moe_slices(448, 3) == [(0, 192), (192, 384), (384, 448)]
    for mt in (1, 2, 4, 8):          # every N and both row sources with every MT, and with every (K, split)
        assert {c[4] for c in cases if mp.moe_mt(c[0]) == mt} == set(mp.MOE_NS)
        assert {c[5] for c in cases if mp.moe_mt(c[0]) == mt} == set(mp.MOE_SRC_DIVS)
    for ks in mp.MOE_KS:
        assert {c[4] for c in cases if (c[2], c[3]) == ks} == set(mp.MOE_NS)
        assert {c[5] for c in cases if (c[2], c[3]) == ks} == set(mp.MOE_SRC_DIVS)
    counts = {(mp.moe_mt(c[0]), n) for c in cases for n in c[1]}
    assert {(1, 0), (1, 1), (1, 7), (1, 16), (4, 64), (4, 33), (8, 128), (8, 129), (8, 257), (8, 37)} <= counts
    chunks = {-(-c[0] // 128) for c in cases if mp.moe_mt(c[0]) == 8}
    assert chunks == {1, 2, 3}
    for c in cases:                   # never an index outside [0, max_rows); the decoy is a row of no expert
        A, W, cnt, lists, decoy = mp.moe_inputs(c)
        assert int(lists.min()) >= 0 and int(lists.max()) < c[0] and lists.shape == (len(c[1]), c[0])
        listed = torch.cat([lists[e, :n] for e, n in enumerate(c[1])])
        assert listed.unique().numel() == listed.numel() and (decoy is None or decoy not in listed.tolist())
        assert (decoy is None) == (sum(c[1]) == c[0])
    for (K, N, split, with_p) in mp.MOE_REFUSED:
        kps = mp.moe_kps(K, max(split, 1))
        assert K % 64 or N % 4 or split < 1 or (split > 1 and not with_p) or (K + kps - 1) // kps != split


def test_moe_gemm_probe_rejects_every_mutation():
    cases = mp.moe_cases()
    APPLIED = {m: 0 for m in mp.MOE_MUTATIONS}
    for case in cases:
        inp = mp.moe_inputs(case)
        ref = mp.moe_want(case, inp)                   # raises if a slab or a product leaves the bound
        split = case[3]
        what = f"moe_gemm max_rows={case[0]} counts={case[1]} K={case[2]} split={split} N={case[4]} src_div={case[5]}"

        def check(P):
            # what the GPU module reads: Y in bf16 at split 1, the fp32 slabs above it
            mp.assert_moe(P[0].to(gp.BF) if split == 1 else P, ref if split > 1 else ref[0], what)

        base = mp.moe_gemm_emulate(case, inp)
        assert not _rejected(check, base), f"the unmutated emulator fails: {what}"
        for mut in mp.MOE_MUTATIONS:
            if mp.moe_target(mut, case, inp) is None:
                continue
            APPLIED[mut] += 1
            for kk in ((5, 37, 63) if mut == "drop_k" else (0,)):
                bad = mp.moe_gemm_emulate(case, inp, mut, base=base, kk=kk)
                assert _rejected(check, bad), f"{mut} (kk={kk}) passes the probe: {what}"
    assert all(APPLIED[m] for m in mp.MOE_MUTATIONS), APPLIED
    print(f"\nmoe_gemm: {len(cases)} cases; mutations rejected (cases applied to): "
          f"{ {m: APPLIED[m] for m in mp.MOE_MUTATIONS} }")


def test_grouped_schedule_is_a_bijection():
    """The mirror of xcd_logical and tile_of gives every (entry, n-tile) to exactly one workgroup, for
    whole and ragged super-rows, in one pass and in the persistent regime."""
    for cus in (64, 104, 256, 304):
        for entries, tiles_n in ((1, 1), (11, 8), (13, 8), (72, 8), (136, 8), (4 * cus // 8 + 8, 8), (2 * cus + 8, 1), (78 + 8, 3)):
            sched = mp.grouped_schedule(entries, tiles_n, cus)
            flat = sorted(t for s in sched for t in s)
            assert flat == [(m, n) for m in range(entries) for n in range(tiles_n)], (cus, entries, tiles_n)
            assert len(sched) == min(cus, entries * tiles_n)
            assert max(len(s) for s in sched) - min(len(s) for s in sched) <= 1


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
def test_persistent_table_shows_every_workgroup_pattern(cus):
    tab, M = mp._layout(mp.persistent_spec(cus))
    assert len(tab) * 8 > 2 * cus
    n, most_units, most_tiles = mp.grouped_patterns(tab, 8, cus)
    assert all(n.values()) and most_units >= 5 and most_tiles >= 3, (n, most_units, most_tiles)
    holes = [i for i, t in enumerate(tab) if t[2] == 0]
    assert holes[0] == 0 and holes[-1] == len(tab) - 1 and len(tab) // 2 in holes
    mp.check_table(tab, M, mp.PERSIST_GROUPS)
    assert len({t[1] for t in tab if t[2] and t[0] == 1}) > 1      # an expert owns several chunks
    print(f"\n{cus} workgroups: {len(tab)} entries ({len(holes)} unused), {len(tab) * 8} tiles, {M} rows; patterns {n}; "
          f"most units / tiles on one workgroup {most_units} / {most_tiles}")


def test_hand_table_is_what_the_issue_names():
    tab, M = mp._layout(mp.HAND_TABLE)
    mp.check_table(tab, M, mp.HAND_GROUPS)
    assert sorted(t[2] for t in tab if t[2]) == [1, 1, 3, 17, 64, 255, 256]
    assert [t[2] for t in tab if t[0] == 1 and t[2]] == [256, 1]          # an expert over two chunks
    assert 4 not in {t[0] for t in tab if t[2]}                            # an expert with no chunk
    used = torch.zeros(M, dtype=torch.bool)
    for (e, r0, n, _) in tab:
        used[r0:r0 + n] = True
    assert not bool(used[:2].any()) and not bool(used[-3:].any()) and int((~used).sum()) == 10
    assert len(tab) * 8 <= 248                                             # a single pass on an MI355X


@pytest.mark.parametrize("cus", [256])
def test_grouped_probe_rejects_every_mutation(cus):
    cases = mp.grouped_cases(cus)
    applied = {m: 0 for m in mp.GROUPED_MUTATIONS}
    for case in cases:
        d = mp.grouped_inputs(case, cus)
        ref = mp.grouped_want(case, d)                 # raises if a product leaves the bound
        what = f"grouped {case} on {cus} workgroups"
        assert not _rejected(mp.assert_grouped, case, d, mp.grouped_emulate(case, d, cus), ref, what), \
            f"the unmutated emulator fails: {what}"
        for mut in mp.GROUPED_MUTATIONS:
            if not mp.grouped_applies(mut, case, d, cus):
                continue
            applied[mut] += 1
            for kk in ((5, 37, 63) if mut == "drop_k" else (0,)):
                bad = mp.grouped_emulate(case, d, cus, mut, kk=kk)
                assert _rejected(mp.assert_grouped, case, d, bad, ref, what), f"{mut} (kk={kk}) passes the probe: {what}"
        if case[0] == "persistent":                    # the new coverage: every break of the tile walk applies
            assert all(applied[m] for m in ("wrong_expert", "stale_rows", "skip_after_hole", "hole_consumed")), (what, applied)
    assert all(applied.values()), applied
    print(f"\ngrouped, {cus} workgroups: {len(cases)} cases; mutations rejected (cases applied to): {applied}")


def test_order_probe_depends_on_the_order():
    """The order probe's expected answer is the LAST tile's expert per workgroup; a workgroup that ran its
    tiles in the opposite order would leave expert 0's."""
    for cus in (64, 256):
        tab, M, groups, last = mp.order_probe(cus)
        assert len(tab) > 2 * cus and M == 4 * cus and groups == 3 and set(last) == {1, 2}
        for b in (0, cus - 1):
            mine = sorted(t[0] for t in tab if t[1] == 4 * b)
            assert mine == list(range(last[b] + 1))


def test_every_mutation_belongs_to_a_proof():
    """Each proof above asserts that every break of its own list applied to, and was rejected on, at least
    one case; together the two lists are the whole set."""
    assert set(mp.MOE_MUTATIONS) | set(mp.GROUPED_MUTATIONS) == set(mp.MUTATIONS)
    assert {"wrong_expert", "stale_rows", "hole_consumed", "skip_after_hole", "wrap_stored", "sorted_not_slot",
            "gate_up_swap", "src_div_ignored", "short_slice_full", "chunk_clamp", "row_clamp", "drop_k", "drop_step",
            "swap_chunk", "lose_slice", "double_slice"} == set(mp.MUTATIONS)
