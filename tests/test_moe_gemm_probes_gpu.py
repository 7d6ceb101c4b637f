"""The two kernels that do the MoE arithmetic on inputs with exact answers (tests/moe_gemm_probes.py; what
each probe catches is proven on the CPU by tests/test_moe_gemm_probes_cpu.py over the same case lists):
moe_gemm_kernel<MT> through ka_moe_gemm and the grouped gemm256_kernel through ka_gemm_big_grouped, both
called through _hip.require() the way ops.moe_experts and ops.moe_experts_grouped call them.  Every GEMM
comparison is torch.equal against the fp64 product, sentinels of unwritten rows included; SwiGLU outputs
may be one bf16 ulp off.

The grouped kernel's persistent regime (a workgroup runs a second, third, .. tile: the next unit's decode,
unused entries skipped between tiles, the next tile's offsets installed during the current tile's last
trip, the re-stage without a next unit) is run by a table sized from the device: more than 4 x CUs tiles,
with every workgroup pattern of moe_gemm_probes.PATTERNS asserted on the mirror of the launch, and the
mirror's grouping and order of tiles checked by one run whose answer depends on them
(test_grouped_tile_order_matches_the_mirror).

Measured on an MI355X (256 CUs); the module prints these again at teardown (see them with -s):
  * 34 (kernel, MT or epilogue, K, split) combinations: ka_moe_gemm 28 (MT 1, 2, 4, 8 x K 64, 128, 192, 320
    at split 1, 320 at split 2, 448 at split 3, 512 at split 4; 63 cases over 9 row counts), ka_gemm_big_grouped
    6 (bf16 and SwiGLU x K 128, 256, 384; 20 launches over the hand-written, the ka_moe_sort and the
    persistent table) plus the order probe.  Every one exact.
  * SwiGLU outputs one bf16 ulp from the fp64 reference: 0 of 20,885,376 (g and u are small integers, as
    in test_gemm_probes_gpu.py; the allowance stays for another __expf).
  * persistent table on 256 workgroups: 136 entries (46 unused) x 8 n-tiles = 1088 tiles over 5826 sorted
    rows; a workgroup runs up to 5 units and up to 5 tiles.  Workgroups per pattern: unused entry before
    the first tile 61, tile / unused / tile 26, last tile followed by unused entries only 75, tiles of two
    experts back to back 138, two chunks of one expert back to back 43.
  * the order probe (520 one-tile entries, the tiles of a workgroup stacked on one chunk) ends with every
    workgroup's last expert: the kernel groups and orders its units as the mirror says.
  * wall time 1.8 s (20 tests).
"""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU with -m "not gpu" deselected anyway
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from ai_agent_kubectl_amd.ops._hip import check  # noqa: E402
from tests import elementwise_probes as ep  # noqa: E402
from tests import gemm_probes as gp  # noqa: E402
from tests import moe_gemm_probes as mp  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
_p, _st = ops._p, ops._stream
EPI = {"bf16": ops.GB_EPI_BF16, "swiglu": ops.GB_EPI_SWIGLU}
COMBOS = set()                      # (kernel, MT or epilogue, K, split)
ULPS = [0, 0]                       # SwiGLU elements one ulp off, elements
PERSIST = {}                        # the persistent table's facts


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7


@pytest.fixture(autouse=True, scope="module")
def _lib():
    _hip.require()
    t0 = time.time()
    yield
    per = {}
    for c in COMBOS:
        per[c[0]] = per.get(c[0], 0) + 1
    print(f"\n(kernel, MT or epilogue, K, split) combinations run: {len(COMBOS)} {sorted(per.items())}")
    print(f"SwiGLU (grouped gemm_big): {ULPS[0]} of {ULPS[1]} elements one bf16 ulp from the fp64 reference")
    print(f"persistent table: {PERSIST}")
    print(f"module wall time {time.time() - t0:.1f} s")


def _sent(shape, dtype):
    return torch.full(shape, gp.SENTINEL, dtype=dtype, device=DEV)


# ---- ka_moe_gemm -----------------------------------------------------------------------------------
def _moe_gemm(case, inp_d, Y, P):
    mr, cs, K, split, N, sd = case
    A, W, counts, lists = inp_d
    return _hip.require().ka_moe_gemm(_p(Y), _p(A), _p(W), _p(counts), _p(lists), mr, len(cs), N, K, sd, mr, split,
                                      _p(P), _st())


@pytest.mark.parametrize("max_rows", mp.MOE_MAX_ROWS)
def test_moe_gemm_exact(max_rows):
    """Every (K, split) of moe_gemm_probes.MOE_KS at this max_rows (MT = 1, 2, 4, 8; one to three row
    chunks), N = 4 .. 132 and both row sources in turn: Y equals the fp64 product on every listed row and
    the sentinel elsewhere (the decoy row that the list entries past a count name included); with split-K
    every slab equals its slice's product.  The slabs then go through ops.silu_mul(SplitK) and
    ka_moe_combine where N suits them (N % 16 / N % 8): equal to the same functions on the exact slabs."""
    lib = _hip.require()
    fed = 0
    for case in [c for c in mp.moe_cases() if c[0] == max_rows]:
        mr, cs, K, split, N, sd = case
        inp = mp.moe_inputs(case)
        ref = mp.moe_want(case, inp, DEV)
        inp_d = tuple(t.to(DEV) for t in inp[:4])
        what = f"ka_moe_gemm max_rows={mr} (MT {mp.moe_mt(mr)}) counts={cs} K={K} split={split} N={N} src_div={sd}"
        COMBOS.add(("moe_gemm", mp.moe_mt(mr), K, split))
        if split == 1:
            Y = _sent((mr, N), BF)
            check(_moe_gemm(case, inp_d, Y, None), what)
            mp.assert_moe(Y, ref[0], what, 16 * mp.moe_mt(mr))
            continue
        P = _sent((split, mr, N), torch.float32)
        check(_moe_gemm(case, inp_d, None, P), what)
        mp.assert_moe(P, ref, what, 16 * mp.moe_mt(mr))
        exact = ref.float()
        if N % 16 == 0:
            assert torch.equal(ops.silu_mul(ops.SplitK(P, split)), ops.silu_mul(ops.SplitK(exact, split))), what
            fed += 1
        if N % 8 == 0:
            T, k, ids, w = mp.moe_combine_routing(case, inp)
            idd, wd = ids.to(DEV), w.to(DEV)
            outs = []
            for slabs in (P, exact):
                out = _sent((T, N), BF)
                check(lib.ka_moe_combine(_p(out), None, _p(slabs), split, _p(wd), _p(idd), T, k, N, 0,
                                         len(cs), _st()), "moe_combine")
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), what
            # and what the combine makes of them is the weighted sum of the listed rows alone
            want = ep.moe_combine_want(None, exact.cpu(), w, ids, 0, len(cs))
            ep.assert_equal(outs[0], want.to(BF), what + " combined")
    torch.cuda.synchronize()
    assert fed == sum(1 for c in mp.moe_cases() if c[0] == max_rows and c[3] > 1 and c[4] % 16 == 0)


def test_moe_gemm_return_codes():
    """Refused with Y and P untouched: K % 64, N % 4, split < 1, split > 1 without P, a split that leaves
    a slice empty (K = 256 at split 3).  max_rows <= 0 returns 0 and writes nothing."""
    lib = _hip.require()
    mr, el = 16, 2
    counts = torch.tensor([7, 3], dtype=torch.int32, device=DEV)
    lists = torch.arange(mr, dtype=torch.int32, device=DEV).repeat(el, 1).contiguous()
    for (K, N, split, with_p) in mp.MOE_REFUSED:
        A = gp.make_x(mr, K, 1).to(DEV)
        W = torch.zeros((el, N, K), dtype=BF, device=DEV)
        Y, P = _sent((mr, N), BF), _sent((max(split, 1), mr, N), torch.float32)
        rc = lib.ka_moe_gemm(_p(Y), _p(A), _p(W), _p(counts), _p(lists), mr, el, N, K, 1, mr, split,
                             _p(P) if with_p else None, _st())
        torch.cuda.synchronize()
        assert rc != 0, (K, N, split, with_p)
        assert bool((Y == gp.SENTINEL).all()) and bool((P == gp.SENTINEL).all()), (K, N, split, with_p)
    A, W = gp.make_x(mr, 64, 1).to(DEV), torch.zeros((el, 64, 64), dtype=BF, device=DEV)
    Y = _sent((mr, 64), BF)
    for rows in (0, -1):
        assert lib.ka_moe_gemm(_p(Y), _p(A), _p(W), _p(counts), _p(lists), mr, el, 64, 64, 1, rows, 1, None, _st()) == 0
    torch.cuda.synchronize()
    assert bool((Y == gp.SENTINEL).all())


# ---- ka_gemm_big_grouped ---------------------------------------------------------------------------
def _grouped(case, d, X=None, tab=None, out_rows=None):
    """One launch into a sentinel-filled Y, the way ops.moe_experts_grouped calls the entry point."""
    kind, epi, K, width = case
    lib = _hip.require()
    X = d["X"].to(DEV) if X is None else X
    W = d["W"].to(DEV)
    tab = torch.tensor(d["tab"], dtype=torch.int32, device=DEV).flatten() if tab is None else tab
    M, groups = d["M"], d["groups"]
    assert X.shape == (M, K) and tab.numel() == 4 * len(d["tab"]) and W.shape[0] == groups
    if epi == "swiglu":
        Y = _sent((M, width), BF)
        check(lib.ka_gemm_big_grouped(_p(Y), _p(X), _p(W), _p(tab), len(d["tab"]), None, M, 2 * width, K, K, width, groups,
                                      EPI[epi], _st()), f"gemm_big_grouped {case}")
    else:
        out_rows = d["out_rows"].to(DEV) if out_rows is None else out_rows
        assert out_rows.numel() == M and int(out_rows.max()) < d["Yrows"] and int(out_rows.min()) >= 0
        Y = _sent((d["Yrows"], width), BF)
        check(lib.ka_gemm_big_grouped(_p(Y), _p(X), _p(W), _p(tab), len(d["tab"]), _p(out_rows), M, width, K, K, width,
                                      groups, EPI[epi], _st()), f"gemm_big_grouped {case}")
    COMBOS.add(("gemm_big_grouped", epi, K, 1))
    return Y


def _check_grouped(case, d, Y, what):
    one, tot = mp.assert_grouped(case, d, Y, mp.grouped_want(case, d, DEV), what)
    ULPS[0] += one
    ULPS[1] += tot


@pytest.mark.parametrize("K", mp.GROUPED_KS)
def test_grouped_hand_written_table_exact(K):
    """moe_gemm_probes.HAND_TABLE, a single pass (at most one tile per workgroup, asserted): chunks of 256,
    1, 3, 17, 64, 255 and 1 rows, an expert over two chunks, an expert with none, unused entries at the
    start, in the middle and at the end, gaps of sorted rows between chunks and Y rows that no out_rows
    entry names (all keep the sentinel), K = 1, 2 and 3 trips, both epilogues, both widths."""
    cus = _cus()
    for case in [c for c in mp.grouped_cases(cus) if c[0] == "hand" and c[2] == K]:
        d = mp.grouped_inputs(case, cus)
        assert len(d["tab"]) * mp.tiles_n_of(case[1], case[3]) <= cus
        _check_grouped(case, d, _grouped(case, d), f"grouped {case}")


def test_grouped_table_from_moe_sort_exact():
    """The layout ka_moe_sort itself makes of elementwise_probes.MOE_ROUTINGS[1026] (8 chunks, the 5 unused
    entries at the end of the table), produced by the kernel and checked against moe_sort_want, then run
    through both epilogues with the kernel's own table, sorted rows and slots."""
    lib = _hip.require()
    cus = _cus()
    x, counts, lists, sd, chunks = mp.sorted_routing()
    R, K = mp.SORTED_R, mp.SORTED_K
    xs = torch.full((R, K), ep.SENT, dtype=BF, device=DEV)
    slot = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    tab = torch.full((chunks * 4,), -1, dtype=torch.int32, device=DEV)
    xd, cd, ld = x.to(DEV), counts.to(DEV), lists.to(DEV)
    check(lib.ka_moe_sort(_p(xs), _p(slot), _p(tab), _p(xd), _p(cd), _p(ld), R, sd, K, len(counts), chunks, _st()),
          "moe_sort")
    ep.assert_sort(xs, slot, tab, ep.moe_sort_want(x, counts, lists, sd, chunks), "moe_sort for the grouped probe")
    for case in [c for c in mp.grouped_cases(cus) if c[0] == "sorted"]:
        d = mp.grouped_inputs(case, cus)
        assert len(d["tab"]) == chunks and chunks * mp.tiles_n_of(case[1], case[3]) <= cus
        _check_grouped(case, d, _grouped(case, d, X=xs, tab=tab, out_rows=slot), f"grouped {case}")


@pytest.mark.parametrize("K", mp.GROUPED_KS)
def test_grouped_persistent_table_exact(K):
    """More tiles than 2 x CUs (asserted), so workgroups run up to five units: the table of
    moe_gemm_probes.persistent_spec for this device, on which the mirror of the launch shows a workgroup
    that skips an unused entry before its first tile, one that skips one between two tiles, one whose last
    tile is followed only by unused entries, one that runs tiles of two experts back to back and one that
    runs two chunks of one expert back to back (all asserted).  At K = 128 a tile's only trip is its last:
    the next tile's offsets are installed before any MFMA of the current one."""
    cus = _cus()
    for case in [c for c in mp.grouped_cases(cus) if c[0] == "persistent" and c[2] == K]:
        d = mp.grouped_inputs(case, cus)
        tiles_n = mp.tiles_n_of(case[1], case[3])
        tiles = len(d["tab"]) * tiles_n
        assert tiles > 2 * cus, (tiles, cus)
        n, most_units, most_tiles = mp.grouped_patterns(d["tab"], tiles_n, cus)
        assert all(n.values()) and most_tiles >= 2, (n, most_tiles)
        holes = [i for i, t in enumerate(d["tab"]) if t[2] == 0]
        assert holes[0] == 0 and holes[-1] == len(d["tab"]) - 1 and len(d["tab"]) // 2 in holes
        PERSIST.update(cus=cus, entries=len(d["tab"]), unused=len(holes), tiles=tiles, rows=d["M"],
                       most_units_per_workgroup=most_units, most_tiles_per_workgroup=most_tiles, patterns=n)
        _check_grouped(case, d, _grouped(case, d), f"grouped {case} ({tiles} tiles on {cus} workgroups)")


def test_grouped_tile_order_matches_the_mirror():
    """moe_gemm_probes.order_probe: the tiles the mirror gives one workgroup all write the same 3 rows,
    each with another expert, so the rows end up holding the answer of the workgroup's last tile."""
    lib = _hip.require()
    cus = _cus()
    tab, M, groups, last = mp.order_probe(cus)
    assert len(tab) > 2 * cus and min(last) >= 1
    K, N = 128, 256
    X = gp.make_x(M, K, 31337).to(DEV)
    W = mp._weights("bf16", groups, N, K).to(DEV)
    want = torch.full((M, N), gp.SENTINEL, dtype=torch.float64, device=DEV)
    for b, e in enumerate(last):
        want[4 * b:4 * b + 3] = gp.want(X[4 * b:4 * b + 3], W[e])
    Y = _sent((M, N), BF)
    tabd = torch.tensor(tab, dtype=torch.int32, device=DEV).flatten()
    rows = torch.arange(M, dtype=torch.int32, device=DEV)
    check(lib.ka_gemm_big_grouped(_p(Y), _p(X), _p(W), _p(tabd), len(tab), _p(rows), M, N, K, K, N, groups,
                                  ops.GB_EPI_BF16, _st()), "gemm_big_grouped (order probe)")
    gp.assert_exact(Y, want, f"order probe: {len(tab)} one-tile entries on {cus} workgroups (row 4 b + i = workgroup b)", 4, N)


def test_grouped_return_codes():
    """Refused with Y all sentinel: N % 256, K % 128, ldx or ldy no multiple of 8, groups < 1, a null
    table, EPI_BF16 without out_rows, an epilogue other than 0 and 3.  chunks <= 0, M <= 0 and a table of
    unused entries only return 0 and write nothing."""
    lib = _hip.require()
    M, N, K, groups = 8, 256, 128, 2
    X = gp.make_x(M, K, 2).to(DEV)
    W = torch.ones((groups, N, K), dtype=BF, device=DEV)
    tab = torch.tensor([0, 0, 8, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    rows = torch.arange(M, dtype=torch.int32, device=DEV)
    Y = _sent((M, N + 8), BF)

    def call(N=N, K=K, ldx=K, ldy=N, groups=groups, tab=tab, rows=rows, epi=0, chunks=2, M=M):
        rc = lib.ka_gemm_big_grouped(_p(Y), _p(X), _p(W), _p(tab), chunks, _p(rows), M, N, K, ldx, ldy, groups, epi, _st())
        torch.cuda.synchronize()
        assert bool((Y == gp.SENTINEL).all()), "a refused or empty launch wrote Y"
        return rc

    for kw in (dict(N=128), dict(N=384), dict(K=64), dict(K=192), dict(ldx=K + 4), dict(ldy=N + 4), dict(groups=0),
               dict(tab=None), dict(rows=None), dict(epi=1), dict(epi=2), dict(epi=4), dict(epi=5)):
        assert call(**kw) != 0, kw
    assert call(epi=ops.GB_EPI_SWIGLU, rows=None, tab=None) != 0
    for kw in (dict(chunks=0), dict(chunks=-1), dict(M=0), dict(M=-3), dict(tab=torch.zeros(8, dtype=torch.int32, device=DEV)),
               dict(tab=torch.zeros(8, dtype=torch.int32, device=DEV), epi=ops.GB_EPI_SWIGLU, rows=None)):
        assert call(**kw) == 0, kw
    # the same operands launch once nothing is wrong with them (Y's row stride is N + 8)
    check(lib.ka_gemm_big_grouped(_p(Y), _p(X), _p(W), _p(tab), 2, _p(rows), M, N, K, K, N + 8, groups, 0, _st()), "valid")
    gp.assert_exact(Y[:, :N], gp.want(X, W[0]), "the valid launch after the refusals")
    assert bool((Y[:, N:] == gp.SENTINEL).all())


def test_moe_block_big_path_with_more_tiles_than_workgroups(monkeypatch):
    """ops.moe_experts_grouped on the gemm_big path at H = 512, I = 384 with enough tokens that the
    gate_up launch has more tiles than workgroups (asserted), against the dense fp32 reference at the
    tolerance of the other block tests.  The exact probes above are the sharp check; this one runs the
    wrapper's own tables and buffers in the multi-tile regime."""
    monkeypatch.setattr(ops, "MOE_PREFILL", "big")
    cus = _cus()
    E, H, I, k = 8, 512, 384, 2
    T = 128 * (cus // 3 - E + 1)
    assert (-(-2 * T // 256) + E) * (I // 128) > cus and ops.moe_big_ok(H, I, E, T * k)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, H, generator=g).to(BF).to(DEV)
    w13 = (torch.randn(E, 2 * I, H, generator=g) * 0.05).to(BF).to(DEV)
    w2 = (torch.randn(E, H, I, generator=g) * 0.05).to(BF).to(DEV)
    tw, tid = ops.moe_topk(torch.randn(T, E, generator=g).to(BF).to(DEV), k)
    ring = []
    monkeypatch.setattr(ops, "linear_grouped", lambda *a, **kw: ring.append(1))
    got = ops.moe_experts_grouped(x, w13, w2, tw, tid, 0)
    assert not ring                                       # the gemm_big path, not the ring kernel
    torch.testing.assert_close(got.float(), ep.moe_dense_ref(x, w13, w2, tw, tid, 0), atol=5e-2, rtol=5e-2)
