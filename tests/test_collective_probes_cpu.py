"""The probes of tests/collective_probes.py can fail: at every case of the list
tests/test_collective_probes_gpu.py walks (it runs worlds 2, 3 and 4), at world 2, 3, 4 and 8, a torch emulation of the kernels of csrc/allreduce.hip passes the probe as
it is and is rejected with each of these breaks built in:

    every kernel       the last rank dropped, rank 0 read in place of the last rank, every peer pointer the
                       rank's own, the peers' other half (the call before) read
    all-reduce, gather chunk not rounded to 8 elements (the last vector runs past n), the ragged last chunk
                       not handled, only the first 4096-element pass of a workgroup done
    all-gather         rank order reversed, the staging's padding not cut out of every row
    fused RMSNorm      rank sum kept in fp32 into the residual add, residual written back unrounded
                       (truncated, and the norm fed the unrounded sum), residual ignored, norm of the sum
                       without the residual, last slab dropped, last slab doubled, rows per workgroup floored,
                       second 512-vector slot lost, the row's last vector missing from the sum of squares

The walk keeps the emulation's halves from call to call, as the GPU run does, so "the other half" holds
what the call before really left there.  The last two tests keep on record what the comparison of
tests/test_custom_allreduce_gpu.py (max |got - want| < 0.1 on randn) lets through.
"""
import pytest
import torch

from tests import collective_probes as cp
from tests import elementwise_probes as ep

BF = cp.BF


def _ops(world, kind=None):
    return [o for c in cp.cases(world) for o in c["ops"] if kind is None or o["kind"] == kind]


# ---- the walk: the emulation passes, every mutation is rejected -------------------------------------
@pytest.mark.parametrize("world", cp.WORLDS)
def test_emulation_passes_and_every_mutation_is_rejected(world):
    emus = {"main": cp.Emu(world, cp.CAP), "big": cp.Emu(world, cp.BIG_CAP)}
    stale = {"main": cp.Emu(world, cp.CAP), "big": cp.Emu(world, cp.BIG_CAP)}
    rejected = {(k, m): 0 for k, muts in cp.MUTATIONS_OF.items() for m in muts}
    nops = 0
    worst = {"free": 0.0, "fused": 0.0}
    for case in cp.cases(world):
        if case["kind"] == "refusals":
            for fn, over in cp.refusals():
                for rank in range(world):
                    a = cp.refusal_args(fn, over, world, rank)
                    assert cp.host_refuses(fn, cap=cp.CAP, **a), (fn, over)
                    base = cp.refusal_args(fn, {}, world, rank)
                    assert not cp.host_refuses(fn, cap=cp.CAP, **base)
                    assert sum(a[k] != base[k] for k in a) <= 2      # one thing wrong (rows and hidden go together)
            continue
        for op in case["ops"]:
            nops += 1
            emu = emus[op["inst"]]
            assert op["call"] == emu.ctr
            data = cp.op_data(op, world)
            for mut in cp.MUTATIONS_OF[op["kind"]]:
                if mut == "stale_half":
                    gots = stale[op["inst"]].launch(op, data, mut)
                else:
                    gots = emu.launch(op, data, mut, commit=False)
                if any(cp.compare(op, data, g)[0] for g in gots):
                    rejected[(op["kind"], mut)] += 1
            gots = emu.launch(op, data)
            rec, ratio = cp.compare(op, data, gots[0])
            assert not rec, rec
            if ratio is not None:
                key = "free" if op["kind"] == "ar" else "fused"
                worst[key] = max(worst[key], ratio)
            for g in gots[1:]:                                     # every rank ends with the same bits as rank 0
                assert g["frame_ok"] and ("in_after" not in g or g["in_after"] is data["ins"][g["rank"]])
                for k in ("out", "res"):
                    if g.get(k) is not None and g[k] is not gots[0][k]:
                        assert torch.equal(g[k].view(torch.int16), gots[0][k].view(torch.int16)), op["name"]
    assert emus["main"].ctr == cp.launches(world) and emus["big"].ctr == cp.launches(world, "big")
    assert worst["free"] <= 1 and worst["fused"] <= 1
    print(f"\nworld {world}: {nops} launches; emulation's largest error / bound: free random {worst['free']:.3f}, "
          f"fused output {worst['fused']:.3f}")
    assert {m for _, m in rejected} == set(cp.MUTATIONS)
    for m in cp.MUTATIONS:                                         # counted per kernel: each must reject on its own
        per = ", ".join(f"{k} {rejected[(k, m)]}" for k in cp.MUTATIONS_OF if (k, m) in rejected)
        print(f"  {m:20s} rejected by launches of: {per}")
    assert all(rejected.values()), {k: v for k, v in rejected.items() if not v}


# ---- the side conditions the exactness rests on -----------------------------------------------------
def test_ledger_is_exact_and_tells_ranks_calls_and_positions_apart():
    n = 1 << 16
    i = torch.arange(cp.BIG_N)
    k = cp.ledger_k(i)
    assert int(k.min()) == 0 and int(k.max()) == 15
    kv = k.view(-1, 8)
    nv = kv.shape[0]
    for d in list(range(1, 1100)) + [2048, 4096, 8191, 8192, 65535]:      # shifts in 8-vectors, up to a chunk and beyond
        if d < nv:
            assert bool((kv[d:] != kv[:nv - d]).any(1).all()), d
    for world in cp.WORLDS:
        seen = set()
        for call in range(8):
            parts = torch.stack([cp.ledger(n, p, call) for p in range(world)])
            assert bool((parts != 0).all())
            s = cp.exact_sum(parts, "ledger")                          # order-independent in fp32
            want = cp.ledger_sum(n, world, call)
            assert torch.equal(want.double(), s)                       # and exact in bf16
            e = torch.log2(parts.float().abs())
            assert float(e.min()) >= -32 and float(e.max()) <= 39
            for bad in (parts[:-1], torch.cat([parts[:-1], parts[:1]]), parts[:1].repeat(world, 1)):
                assert bool((bad.double().sum(0) != s).all())          # lost, doubled, own rank only: every element
            seen.add(float(want[0]))
        assert len(seen) == 4                                          # calls c .. c + 3 differ, c + 4 repeats


def test_bounded_random_is_exact_in_fp32_and_rounds_in_bf16():
    for world in cp.WORLDS:
        parts = torch.stack([cp.bounded_randn((1 << 14,), ep.case_seed(world, p)) for p in range(world)])
        a = parts.float().abs()
        assert float(a.min()) >= 2.0 ** -10 and float(a.max()) < 2
        s = cp.exact_sum(parts, "bounded")
        inexact = float((s.to(BF).double() != s).float().mean())
        assert 0.5 < inexact < 0.9, inexact                            # the rounding to bf16 is a real one
        # the alternatives the family exists to catch
        acc = parts[0]
        for p in range(1, world):
            acc = (acc.float() + parts[p].float()).to(BF)              # accumulated in bf16
        trunc = cp._trunc_bf16(s.float())
        assert not torch.equal(trunc, s.to(BF)) and (world == 2 or not torch.equal(acc, s.to(BF)))
        slabs = cp.bounded_randn((9, 1 << 12), ep.case_seed(world, 99), hi=1.0)
        assert float(slabs.float().abs().max()) < 1 and float(cp.exact_sum(slabs, "slabs").abs().max()) < 9


def test_fused_inputs_are_exact_and_probe_what_they_claim():
    for world in (2, 8):
        for op in _ops(world, "fused"):
            probe_rows = op["rows"] == len(cp.fused_probe_positions(op["hidden"])) and world == 2
            if op["rows"] > 3 and not (op["rows"] == 65 and op["split"] > 1) and not probe_rows:
                continue
            d = cp.op_data(op, world)
            rows, hidden, split = op["rows"], op["hidden"], op["split"]
            assert len(d["ins"]) == world
            for t in d["ins"]:
                assert t.shape == ((split, rows, hidden) if split > 1 else (rows, hidden))
                assert t.dtype == (BF if op["slab_bf16"] else torch.float32)
                assert bool((t.reshape(-1, 8) != 0).any(1).all())      # a dropped rank or slab shows in every vector
            staged = torch.stack([cp.stage_slabs(t, split) for t in d["ins"]])
            assert torch.equal(staged, d["contrib"])
            assert bool((d["want"] != 0).any())
            if op["family"] == "int":
                assert float(d["xsum"].float().abs().max()) in (127.0, 128.0, 129.0)
            if probe_rows:                                             # one row per position, each carrying the +-128
                pos = torch.tensor(cp.fused_probe_positions(hidden))
                assert bool((d["xsum"].float()[torch.arange(rows), pos].abs() >= 127).all())
            if op["with_res"] and op["family"] != "ledger" and rows * hidden > 8:
                assert not torch.equal(d["want_res"].double(), d["xsum"].double() + d["res"].double())   # the add rounds
            if op["family"] == "bounded" and rows * hidden > 8:
                tot = d["contrib"].double().sum(0)
                assert not torch.equal(tot.to(BF).double(), tot)       # the rank sum rounds


# ---- the case list covers what it claims ------------------------------------------------------------
@pytest.mark.parametrize("world", cp.WORLDS)
def test_case_list_coverage(world):
    ops = _ops(world)
    nb = cp.max_blocks(world)
    assert nb == (32 if world == 8 else 64)
    assert all(world * o["nblocks"] <= 256 for o in ops)
    names = [o["name"] for o in ops]
    assert len(set(names)) == len(names)
    ar = [o for o in ops if o["kind"] == "ar"]
    wrap = [o for o in ar if o["via"] == "wrapper" and not o["name"].startswith(("seq", "graph"))]
    assert {(o["n"], o["nblocks"], cp.chunk_of(o["n"], o["nblocks"])) for o in wrap} == {
        (8, 1, 8), (4096, 1, 4096), (4104, 2, 2056), (12296, 4, 3080), (65536, 16, 4096)}
    assert {o["family"] for o in wrap} == {"ledger", "bounded", "free"}
    assert any(o["n"] == cp.CAP for o in wrap)
    direct = [o for o in ar if o["via"] == "direct"]
    assert all(o["framed"] for o in direct)
    empty = [o for o in direct if cp.chunk_of(o["n"], o["nblocks"]) * (o["nblocks"] - 1) >= o["n"]]
    assert {(o["n"], o["nblocks"]) for o in empty} == {(8, 3), (8, nb), (72, nb)}     # trailing workgroups own nothing
    multipass = [o for o in direct if cp.chunk_of(o["n"], o["nblocks"]) > cp.PASS]
    assert any(o["n"] == 4104 and o["nblocks"] == 1 for o in multipass)
    big = [o for o in ar if o["inst"] == "big"]
    assert len(big) == (2 if world == 2 else 0)
    assert all((o["inst"] == "big") == (o["kind"] == "fused" and o["rows"] * o["hidden"] > cp.CAP) for o in ops if o not in big)
    for o in big:
        assert o["n"] == 64 * 4096 * 2 + 8 and o["nblocks"] == 64 and cp.chunk_of(o["n"], 64) == 8200 and o in multipass
        assert 63 * 8200 < o["n"] <= cp.BIG_CAP                    # all 64 workgroups own elements, three passes each
    ag = [o for o in ops if o["kind"] == "ag"]
    nbytes = {o["nbytes"] for o in ag if o["via"] == "wrapper"}
    assert nbytes >= {4, 8, 16, 24, 1120}
    assert {b % 16 == 0 for b in nbytes} == {True, False}           # both padding branches
    assert {o["dtype"] for o in ag if o["via"] == "wrapper"} == {torch.int32, torch.float32, BF}
    assert {(o["n16"], o["nblocks"]) for o in ag if o["via"] == "direct" and not o["name"].startswith("seq")} == {
        (4104, 2), (12296, 4), (4104, 1)}
    fused = [o for o in ops if o["kind"] == "fused" and o["family"] != "ledger"]
    probe_shapes = {(len(cp.fused_probe_positions(h)), h) for h in cp.FUSED_PROBE_HIDDENS}
    assert {(o["rows"], o["hidden"]) for o in fused} == set(cp.FUSED_SHAPES) | probe_shapes
    for h in cp.FUSED_PROBE_HIDDENS:                                # every slot boundary and the row's ends get a row
        assert {0, 7, 8, 4095, 4096, 4103, h - 8, h - 1} <= set(cp.fused_probe_positions(h))
    assert any(q // 8 >= 512 + 64 for q in cp.fused_probe_positions(8192))         # waves of the second slot
    deep = {(o["split"], o["slab_bf16"]) for o in fused if o["family"] == "int" and o["rows"] > o["nblocks"]}
    assert deep == {(1, True)} | {(s, b) for s in cp.FUSED_SPLITS for b in (False, True)}   # all at rows per workgroup > 1
    assert {o["hidden"] // 8 for o in fused} >= {1, 513, 1024}
    for fam in ("int", "bounded"):
        sp = {(o["split"], o["slab_bf16"]) for o in fused if o["family"] == fam}
        assert any(s == 1 for s, _ in sp) and any(1 < s < 4 for s, _ in sp) and any(s > 4 for s, _ in sp)
    assert {(o["split"], o["slab_bf16"]) for o in fused if o["family"] == "int"} == (
        {(1, True)} | {(s, b) for s in cp.FUSED_SPLITS for b in (False, True)})
    for key in {(o["rows"], o["hidden"], o["split"], o["slab_bf16"], o["family"]) for o in fused}:
        both = {o["with_res"] for o in fused if (o["rows"], o["hidden"], o["split"], o["slab_bf16"], o["family"]) == key}
        assert both == {True, False}, key                           # with the residual and with residual=None
    rpb = {o["rows"]: (-(-o["rows"] // o["nblocks"]), o["nblocks"]) for o in fused if o["rows"] >= 64}
    if world <= 4:
        assert rpb[65] == (2, 64) and -(-65 // 2) == 33 and rpb[129] == (3, 64) and rpb[64] == (1, 64)
        assert all(o["via"] == "wrapper" for o in fused)
    else:
        assert rpb[65] == (3, 32) and rpb[129] == (5, 32) and rpb[64] == (2, 32)
    seq = [c for c in cp.cases(world) if c["kind"] == "sequence"][0]["ops"]
    assert len(seq) >= 9 and {o["kind"] for o in seq} == {"ar", "ag", "fused"}
    counts = [o["nblocks"] for o in seq]
    assert max(counts) >= 16 and min(counts) == 1
    assert any(a >= 16 and b == 1 for a, b in zip(counts, counts[1:])) and any(a == 1 and b >= 4 for a, b in zip(counts, counts[1:]))
    graph = [c for c in cp.cases(world) if c["kind"] == "graph"][0]["ops"]
    assert [o["kind"] for o in graph] == ["ar", "fused", "ag"] * cp.GRAPH_REPLAYS
    assert len(graph) // cp.GRAPH_REPLAYS % 2 == 1                  # an odd count: the half parity flips per replay
    ref = cp.refusals()
    for fn in ("ar", "ag"):
        assert [o for f, o in ref if f == fn] == [{"n": 12}, {"n": cp.CAP + 8}, {"nblocks": 0}, {"nblocks": 65},
                                                  {"world": 9}, {"rank": "world"}]
    assert len([o for f, o in ref if f == "fused"]) == 10


# ---- what the older comparison lets through ---------------------------------------------------------
def _old_inputs(it, n, world=2):
    g = torch.Generator().manual_seed(1000 + it)
    parts = [torch.randn(n, generator=g).to(BF) for _ in range(world)]
    return parts, sum(p.float() for p in parts)


def test_old_comparison_passes_a_scaled_result():
    """test_oneshot_allreduce_two_ranks_one_gpu: randn, max |got - want| < 0.1.  Every element scaled by
    1 + 2^-8 (a whole bf16 ulp, a second rounding and more) stays under it at each of that test's sizes; the
    bounded-random family rejects the same scaling."""
    for it, n in enumerate([8, 4096, 8192 * 8, 4096 * 256, 1 << 20, 16]):
        parts, want = _old_inputs(it, n)
        got = (want * (1 + 2.0 ** -8)).to(BF)
        assert not torch.equal(got, want.to(BF))
        err = float((got.float() - want).abs().max())
        assert err < 0.1, (n, err)
    op = dict(name="scaled", kind="ar", family="bounded", framed=False, n=4096, sid=0, call=0)
    data = cp.op_data(op, 2)
    scaled = (data["want"].float() * (1 + 2.0 ** -8)).to(BF)
    assert cp.compare(op, data, dict(rank=0, out=scaled))[0]
    assert not cp.compare(op, data, dict(rank=0, out=data["want"]))[0]


def test_old_comparison_passes_lost_contributions_but_not_a_whole_vector():
    """Same test, in place: where a contribution of the peer is lost the error is the peer's value there.
    About 8 % of the elements of every size hold a peer value below 0.1, so a peer lost in any of them, or in
    all of them at once, passes; so does a sum truncated to bf16 where it should be rounded.  A whole 8-vector
    left unreduced does not pass on those inputs (the quietest vector of the largest size still has an element
    above 0.1), which is the one thing the old comparison could see.  The ledger rejects a lost element, a
    lost vector and a truncation-sized error wherever they are."""
    for it, n in enumerate([8, 4096, 8192 * 8, 4096 * 256, 1 << 20, 16]):
        parts, want = _old_inputs(it, n)
        peer = parts[1].float()
        quiet = peer.abs() < 0.1
        got = torch.where(quiet, parts[0].float(), want).to(BF)        # the peer never added where it is quiet
        err = float((got.float() - want).abs().max())
        assert err < 0.1, (n, err)
        trunc = cp._trunc_bf16(want)
        assert float((trunc.float() - want).abs().max()) < 0.1
        if n >= 4096:
            assert 0.06 < float(quiet.float().mean()) < 0.1 and not torch.equal(got, want.to(BF))
            assert not torch.equal(trunc, want.to(BF))
            assert float(peer.view(-1, 8).abs().max(1).values.min()) > 0.1   # a whole lost vector is seen
    op = dict(name="lost", kind="ar", family="ledger", framed=False, n=4096, sid=0, call=0)
    data = cp.op_data(op, 2)
    for v in (0, 17, 511):
        got = data["want"].clone()
        got[8 * v:8 * v + 8] = data["ins"][0][8 * v:8 * v + 8]
        rec = cp.compare(op, data, dict(rank=0, out=got))[0]
        assert rec and rec[0][2] == 8
        got = data["want"].clone()
        got[8 * v + 3] = data["ins"][0][8 * v + 3]
        rec = cp.compare(op, data, dict(rank=0, out=got))[0]
        assert rec and rec[0][2] == 1 and rec[0][3] == (8 * v + 3,)
