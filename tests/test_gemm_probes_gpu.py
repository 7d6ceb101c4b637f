"""The GEMM kernels of csrc/gemm_mfma.hip, gemm_big.hip and gemm_skinny.hip on inputs with exact answers
(tests/gemm_probes.py; what each probe catches is proven on the CPU by tests/test_gemm_probes_cpu.py):
odd and single k-step counts per split-K slice, configurations 6 and 8, ragged tiles both ways, strided
x, out= views inside a frame of sentinels, gemm_big at its smallest K and with a split tail, the MoE
router's N = 8, the row GEMV at its smallest K and odd N, and the fused LM head on tied integer logits.
Every GEMM comparison is torch.equal against the fp64 product; SwiGLU outputs may be one bf16 ulp off.

Measured on an MI355X (256 CUs); the module prints these again at teardown (see them with -s):
  * 472 (kernel, cfg, k-steps per slice, split, epilogue) combinations: linear_gm 304 (8 configurations
    x nk 1, 2, 3, 5, 7 x {split 1 bf16; split 2 and 4 reduced, deferred fp32, deferred bf16}, and nk 7 at
    split 8), grouped 24, ring SwiGLU 30, gemm_big 15 (4 of them on the
    192-wide tile) + 6 with a split tail, gemm_skinny 27, gemv_rows
    60, swiglu_linear 6.  Every one exact.
  * SwiGLU outputs one bf16 ulp from the fp64 reference: 0 of 1,849,920 (gemm_mfma) and 0 of
    110,932,992 (gemm_big).  g and u are small integers, so silu(g) * u takes few distinct values and
    none of them sits within fp32 error of a bf16 rounding boundary; the one-ulp allowance stays for
    another __expf.
  * gemm_big split tail (M = 8193, N = 2048: 264 tiles on 256 CUs, 8 in the tail), plain and SwiGLU
    epilogues alike: K = 768 two slices of 3 trips, K = 896 slices of 3 and 4 trips, K = 1024 two of 4.
    Below K = 768 the planner does not split (choose_tail's cost model), and a one-trip slice never wins
    at any K.
  * N = 192 is refused by gemm_big (N % 128 != 0), and at N = 384 choose_tn keeps the 256-wide tile for
    every M up to 600, so the 192-wide tile (TN 6) runs at gemm_probes.BIG_TN6_SHAPES, where
    ka_gemm_big_tn returns 6 (asserted), over the same K set.
  * wall time 4.3 s (114 tests) next to about 155 s for the rest of the GPU suite.

The reduce of gemv_rows' slabs takes its scalar variant whenever M * N is no multiple of 4
(csrc/gemm_skinny.hip ka_splitk_reduce_launch): test_gemv_rows_exact runs it at N = 1, 3 and 4 rw + 1,
down to a single output element.
"""
import functools
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU with -m "not gpu" deselected anyway
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import gemm_probes as gp  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
COMBOS = set()                      # (kernel, cfg, k-steps per slice, split, epilogue)
ULPS = {}                           # kernel -> [elements one ulp off, elements]
TAILS = []                          # gemm_big split-tail cases that ran
SWIGLU_CFGS = tuple(c for c in gp.GM_ALL_CFGS if gp.GM_TN[c] % 2 == 0 and c != 19)


@pytest.fixture(autouse=True, scope="module")
def _lib():
    lib = _hip.require()
    torch.manual_seed(0)
    for cfg, (bn, bm) in gp.GM_TILES.items():
        assert (lib.ka_gm_bn(cfg), lib.ka_gm_bm(cfg)) == (bn, bm), cfg
    plan = dict(ops.GEMM_PLAN)
    t0 = time.time()
    yield
    assert ops.GEMM_PLAN == plan
    per = {}
    for c in COMBOS:
        per[c[0]] = per.get(c[0], 0) + 1
    print(f"\n(kernel, cfg, nk, split, epilogue) combinations run: {len(COMBOS)} {sorted(per.items())}")
    for k, (one, tot) in sorted(ULPS.items()):
        print(f"SwiGLU {k}: {one} of {tot} elements one bf16 ulp from the fp64 reference ({one / max(tot, 1):.2e})")
    print(f"gemm_big split-tail cases (M, N, K, epi, slices, trips per slice): {TAILS}")
    print(f"module wall time {time.time() - t0:.1f} s")


def _ulps(kernel, got, ref, what, bm, bn):
    one, tot = gp.assert_swiglu(got, ref, what, bm, bn)
    acc = ULPS.setdefault(kernel, [0, 0])
    acc[0] += one
    acc[1] += tot


def _x_variants(x):
    return (("contiguous x", x), ("strided x", gp.strided(x)))


# ---- ring and ping-pong kernels --------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _gm_inputs(M, N, K, split):
    """(x, w, fp64 slabs, fp64 product) on the GPU, shared by the configurations that run one shape."""
    x, w = gp.make_xw(M, N, K, gp.case_seed(M, N, K, 0))
    slabs = gp.want_slabs(x, w, gp.even_slices(K, split))
    return x.to(DEV), w.to(DEV), slabs.to(DEV), gp.want(x, w).to(DEV)


def _gm_case(cfg, M, N, K, split):
    bn, bm = gp.GM_TILES[cfg]
    # one input set: tests/test_gemm_probes_cpu.py proves the mutations rejected by the draws of draw_seeds
    assert gp.draw_seeds(M, N, K, bm, bn) == [gp.case_seed(M, N, K, 0)]
    x, wd, slabs, ref = _gm_inputs(M, N, K, split)
    nk = K // split // 64
    for tag, xd in _x_variants(x):
        what = f"linear_gm cfg={cfg} M={M} N={N} K={K} nk={nk} split={split} {tag}"
        if split == 1:
            gp.assert_exact(ops.linear_gm(xd, wd, cfg, 1), ref, what + " bf16", bm, bn)
            COMBOS.add(("gm", cfg, nk, 1, "bf16"))
            continue
        gp.assert_exact(ops.linear_gm(xd, wd, cfg, split), ref, what + " reduced fp32 slabs", bm, bn)
        for pb in (False, True):
            sk = ops.linear_gm(xd, wd, cfg, split, defer_reduce=True, bf16_partials=pb)
            name = "deferred bf16 slabs" if pb else "deferred fp32 slabs"
            assert isinstance(sk, ops.SplitK) and sk.split == split and sk.is_bf16 == pb, what
            gp.assert_slabs_exact(sk.P, ref, f"{what} {name}", bm, bn)
            if not torch.equal(sk.P.double(), slabs):
                for s in range(split):
                    gp.assert_exact(sk.P[s], slabs[s], f"{what} {name}, slab {s}", bm, bn)
        COMBOS.update({("gm", cfg, nk, split, e) for e in ("p32+reduce", "p32", "p16")})


@pytest.mark.parametrize("ni", [0, 1])
@pytest.mark.parametrize("mi", [0, 1, 2])
@pytest.mark.parametrize("nk", gp.GM_NKS)
def test_ring_kernels_exact(nk, mi, ni):
    """linear_gm, every configuration (6 and 8 included): nk k-steps per slice (1: shorter than the
    ring's prologue; odd: the last stage changes its issuing wave set), split 1 / 2 / 4, M = 1, BM - 1,
    BM + 1 and N = 16, BN + 16 (mi, ni index gemm_probes.gm_rows / gm_cols), bf16 output, in-kernel
    reduced and deferred fp32 / bf16 slabs, contiguous and strided x."""
    for cfg in gp.GM_ALL_CFGS:
        for split in gp.GM_SPLITS:
            _gm_case(cfg, gp.gm_rows(cfg)[mi], gp.gm_cols(cfg)[ni], 64 * nk * split, split)


@pytest.mark.parametrize("M,N,K,split", gp.GM_TP_SHAPES)
def test_ring_kernels_tp_shard_shapes(M, N, K, split):
    """The TP = 8 shard shapes whose autotune candidates run 7 k-steps per slice, at the plan's rows."""
    for cfg in gp.GM_ALL_CFGS:
        _gm_case(cfg, M, N, K, split)


@pytest.mark.parametrize("mi", [0, 1, 2])
@pytest.mark.parametrize("nk", gp.GM_NKS)
def test_ring_swiglu_one_ulp(nk, mi):
    """linear_gm_swiglu over the model's [gate; up] layout, every configuration with an even TN: I = 16
    and BN / 2 + 16, contiguous x with its own output, strided x into an out= view framed by sentinels."""
    K = 64 * nk
    for cfg in SWIGLU_CFGS:
        bn, bm = gp.GM_TILES[cfg]
        M = gp.gm_rows(cfg)[mi]
        for I in (16, bn // 2 + 16):
            x, w13 = gp.make_swiglu(M, I, K, gp.case_seed(M, I, K))
            ref = gp.want_swiglu(x, w13).to(DEV)
            xd, wd = x.to(DEV), w13.to(DEV)
            what = f"linear_gm_swiglu cfg={cfg} M={M} I={I} K={K}"
            _ulps("gemm_mfma", ops.linear_gm_swiglu(xd, wd, cfg), ref, what, bm, bn // 2)
            whole, view = gp.framed_out(M, I, DEV)
            got = ops.linear_gm_swiglu(gp.strided(xd), wd, cfg, out=view)
            assert got.data_ptr() == view.data_ptr()
            _ulps("gemm_mfma", view, ref, what + " strided x, out= view", bm, bn // 2)
            gp.assert_frame_intact(whole, what)
            COMBOS.add(("gm_swiglu", cfg, nk, 1, "swiglu"))


def test_ring_swiglu_refuses_odd_tn_and_ping_pong():
    """cfg 6 (TN = 3) has no gate / up tile pairs and cfg 19 no [gate; up] gather: an error, not a run."""
    x, w13 = gp.make_swiglu(8, 64, 128, 1)
    for cfg in (6, 19):
        out = torch.full((8, 64), gp.SENTINEL, dtype=BF, device=DEV)
        with pytest.raises(RuntimeError):
            ops.linear_gm_swiglu(x.to(DEV), w13.to(DEV), cfg, out=out)
        torch.cuda.synchronize()
        assert bool((out == gp.SENTINEL).all())


@pytest.mark.parametrize("src_div", [1, 2])
@pytest.mark.parametrize("K", [64, 192, 512])
def test_grouped_ring_exact(K, src_div):
    """linear_grouped on test_gemm_mfma_grouped_gather_scatter's layout (an empty group, a group larger
    than a tile, ragged tails), 1 and 3 k-steps, configurations 6 and 8 included, strided x; rows listed
    for no group keep their sentinel."""
    G, N, R = 5, 400, 900
    counts_h = [0, 1, 300, 17, 260]
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(K + src_div))
    lists = torch.zeros(G, R, dtype=torch.int32)
    o = 0
    for e, c in enumerate(counts_h):
        lists[e, :c] = perm[o:o + c]
        o += c
    x = gp.make_x(R // src_div + 1, K, 5)
    w = torch.stack([gp.make_w(N, K, 100 + e) for e in range(G)])
    refs = [gp.want(x[lists[e, :c].long() // src_div], w[e]).to(DEV) for e, c in enumerate(counts_h)]
    lists_d, counts = lists.to(DEV), torch.tensor(counts_h, dtype=torch.int32, device=DEV)
    wd = w.to(DEV)
    untouched = perm[o:].to(DEV).long()
    for cfg in gp.GM_ALL_CFGS:
        bn, bm = gp.GM_TILES[cfg]
        for tag, xd in _x_variants(x.to(DEV)):
            out = torch.full((R, N), gp.SENTINEL, device=DEV, dtype=BF)
            ops.linear_grouped(xd, wd, counts, lists_d, R, src_div=src_div, cfg=cfg, out=out)
            for e, c in enumerate(counts_h):
                if c:
                    what = f"linear_grouped cfg={cfg} K={K} src_div={src_div} group {e} ({c} rows) {tag}"
                    gp.assert_exact(out[lists_d[e, :c].long()], refs[e], what, bm, bn)
            assert bool((out[untouched] == gp.SENTINEL).all()), (cfg, tag)
        COMBOS.add(("gm_grouped", cfg, K // 64, 1, "bf16"))


# ---- gemm_big --------------------------------------------------------------------------------------
def _gb_plan(M, N, K, epi):
    full, tail = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    ws = ops.gemm_big_ws(torch.device(DEV))
    s = _hip.require().ka_gemm_big_plan(M, N, epi, K, ws.numel(), full.data_ptr(), tail.data_ptr())
    return s, int(full), int(tail)


def _gb_clean():
    """The split tail's counters are back at zero and its error word is clear (as
    test_gemm_big_linear_split_tail_vs_fp32 checks them)."""
    ws = ops.gemm_big_ws(torch.device(DEV))
    assert int(ws[256:256 + 1024 * 32].view(torch.int32).abs().sum()) == 0
    assert ops.gemm_big_err(torch.device(DEV)) == 0


def _gb_bf16_case(xd, wd, ref, tn):
    """linear_big with its own output, then strided x into an out= view framed by sentinels."""
    (M, K), N = xd.shape, wd.shape[0]
    assert gp.draw_seeds(M, N, K, 256, 32 * tn) == [gp.case_seed(M, N, K, 0)]    # one input set, as in _gm_case
    what = f"linear_big M={M} N={N} K={K} (TN {tn}, 256 x {32 * tn} tiles)"
    gp.assert_exact(ops.linear_big(xd, wd), ref, what, 256, 32 * tn)
    whole, view = gp.framed_out(M, N, DEV)
    ops.linear_big(gp.strided(xd), wd, out=view)
    gp.assert_exact(view, ref, what + " strided x, out= view", 256, 32 * tn)
    gp.assert_frame_intact(whole, what)
    COMBOS.add(("big", tn, K // 64, 1, "bf16"))


@pytest.mark.parametrize("K", gp.BIG_KS)
def test_gemm_big_192_wide_tiles_exact(K):
    """gemm256_kernel<EPI_BF16, 6>: the shapes of gemm_probes.BIG_TN6_SHAPES, at which choose_tn picks
    the 192-wide tile (asserted), over the same K set, M = 1, 255, 257, 600, ragged last n-tiles (N is no
    multiple of 192 x 256), contiguous and strided x, out= view with sentinels."""
    lib = _hip.require()
    for (M, N) in gp.BIG_TN6_SHAPES:
        assert lib.ka_gemm_big_tn(M, N, 0) == 6, (M, N)
        x, w = gp.make_xw(M, N, K, gp.case_seed(M, N, K, 0))
        xd, wd = x.to(DEV), w.to(DEV)
        _gb_bf16_case(xd, wd, gp.want(xd, wd), 6)
    _gb_clean()


@pytest.mark.parametrize("M", gp.BIG_MS)
@pytest.mark.parametrize("K", gp.BIG_KS)
def test_gemm_big_small_k_exact(K, M):
    """linear_big and linear_swiglu at K = 128 (one trip: the whole tile is the prologue), 256, 384 (an
    odd number of trips) and 640, N = 128, 384 and 640 on 256-wide tiles (asserted; N = 192 is no multiple of
    128 and must be refused), contiguous x with its own output and strided x into an out= view framed by
    sentinels.  The 192-wide tile has its own test above."""
    lib = _hip.require()
    for N in gp.BIG_NS:
        x, w = gp.make_xw(M, N, K, gp.case_seed(M, N, K, 0))
        ref = gp.want(x, w).to(DEV)
        xd, wd = x.to(DEV), w.to(DEV)
        if N % 128:                          # 192: gemm_big takes whole 128-column blocks only
            assert not ops.big_gemm_ok(xd, wd)
            with pytest.raises(ValueError):
                ops.linear_big(xd, wd)
            continue
        assert lib.ka_gemm_big_tn(M, N, 0) == 8      # the 192-wide tile: test_gemm_big_192_wide_tiles_exact
        _gb_bf16_case(xd, wd, ref, 8)
    for I in gp.BIG_SWIGLU_IS:
        x, w13 = gp.make_swiglu(M, I, K, gp.case_seed(M, I, K))
        ref = gp.want_swiglu(x, w13).to(DEV)
        xd, wd = x.to(DEV), w13.to(DEV)
        what = f"linear_swiglu M={M} I={I} K={K}"
        _ulps("gemm_big", ops.linear_swiglu(xd, wd), ref, what, 256, 128)
        whole, view = gp.framed_out(M, I, DEV)
        ops.linear_swiglu(gp.strided(xd), wd, out=view)
        _ulps("gemm_big", view, ref, what + " strided x, out= view", 256, 128)
        gp.assert_frame_intact(whole, what)
        COMBOS.add(("big", 8, K // 64, 1, "swiglu"))
    x, w13 = gp.make_swiglu(M, 192, K, 3)
    with pytest.raises(ValueError):          # 2I % 256 != 0
        ops.linear_swiglu(x.to(DEV), w13.to(DEV))
    _gb_clean()


def test_gemm_big_split_tail_smallest_k():
    """The split tail at the smallest K the planner gives it.  Candidates: 8 tiles more than one round
    of 256 x 256 tiles fills (M = 32 tile rows + 1 row, N = 8 tiles wide), K = 128 .. 1024, plain and
    SwiGLU epilogues; every candidate the planner splits runs four launches (later launches start from
    the counters the first one reset).  choose_tail's cost model needs 6 trips of 128 to split (s = 2),
    so no slice below K = 512 ever has a single trip, and with s <= trips and s <= 8 a one-trip slice
    never wins; K = 896 (7 trips over 2 slices: 3 and 4) is the uneven case asserted here."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    tm, tn = (cus + 8) // 8, 8
    M = 256 * (tm - 1) + 1
    ran, uneven = 0, 0
    for K in (128, 256, 384, 512, 640, 768, 896, 1024):
        for epi in (0, ops.GB_EPI_SWIGLU):
            N = 256 * tn                              # SwiGLU: w13's 2I rows, a tile is 128 output columns
            s, full, tail = _gb_plan(M, N, K, epi)
            if s <= 1:
                continue
            assert full + tail == tm * tn and tail == 8, (full, tail)
            trips = K // 128
            per = [(k + 1) * trips // s - k * trips // s for k in range(s)]
            assert min(per) >= 1
            if epi:
                x, w = gp.make_swiglu(M, N // 2, K, gp.case_seed(M, N, K))
            else:
                x, w = gp.make_xw(M, N, K, gp.case_seed(M, N, K, 0))
            xd, wd = x.to(DEV), w.to(DEV)
            ref = gp.want_swiglu(xd, wd) if epi else gp.want(xd, wd)     # 16.8 M outputs: fp64 on the GPU
            what = f"split tail M={M} N={N} K={K} epi={epi} s={s} trips per slice {per}"
            for i in range(4):
                if epi:
                    _ulps("gemm_big", ops.linear_swiglu(xd, wd), ref, f"{what} launch {i}", 256, 128)
                else:
                    gp.assert_exact(ops.linear_big(xd, wd), ref, f"{what} launch {i}", 256, 256)
            _gb_clean()
            TAILS.append((M, N, K, "swiglu" if epi else "bf16", s, per))
            COMBOS.add(("big_tail", 8, K // 64, s, "swiglu" if epi else "bf16"))
            ran += 1
            uneven += int(min(per) == 1 or trips % s != 0)
    assert ran and uneven, (ran, uneven, TAILS)


@pytest.mark.parametrize("M", gp.ARGMAX_MS)
@pytest.mark.parametrize("V,K", gp.ARGMAX_VK)
def test_lm_head_argmax_exact(V, K, M):
    """lm_head_argmax on integer logits that tie across 256-token tiles, waves and lanes: the index is
    the lowest allowed global token id among the row's maxima and the value that maximum, exactly; with
    and without masks (row 1 masks the lower copy of many ties), both vocabulary offsets, strided x."""
    x, w = gp.make_argmax_xw(M, V, K, gp.case_seed(M, V, K))
    xd, wd = x.to(DEV), w.to(DEV)
    logits = gp.want(xd, wd)
    midx = torch.tensor([0, 1, -1] * (M // 3 + 1), dtype=torch.int32)[:M]
    for off in gp.ARGMAX_OFFS:
        bits = gp.make_mask(V, off)
        allowed = gp.allowed_tokens(bits, midx, V, off).to(DEV)
        for masked in (False, True):
            wi, wv = gp.expected_argmax(logits, allowed if masked else None, off)
            for tag, xs in _x_variants(xd):
                assert ops.lm_head_argmax_ok(xs, wd, off)
                idx, val = ops.lm_head_argmax(xs, wd, bits.to(DEV) if masked else None,
                                              midx.to(DEV) if masked else None, vocab_offset=off)
                gp.assert_argmax(idx, val, wi, wv, f"lm_head_argmax M={M} V={V} K={K} off={off} masked={masked} {tag}")
    COMBOS.add(("big", 8, K // 64, 1, "argmax"))
    assert ops.gemm_big_err(torch.device(DEV)) == 0


# ---- gemm_skinny -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gp.SKINNY_KS)
@pytest.mark.parametrize("N", gp.SKINNY_NS)
def test_gemm_skinny_exact(N, K):
    """ops.linear(..., split=s) (an explicit split goes to gemm_skinny whatever the plan holds): N below
    and just past the 64-wide tile (8 is the MoE router's), K = 64 (one chunk), 448 (a last slice shorter
    than the others at split 2 and 3) and 4096, plain and deferred."""
    for split in gp.SKINNY_SPLITS:
        sl = gp.skinny_slices(K, split)
        for M in gp.SKINNY_MS:
            for seed in gp.draw_seeds(M, N, K, 256, 64):
                x, w = gp.make_xw(M, N, K, seed)
                slabs, ref = gp.want_slabs(x, w, sl).to(DEV), gp.want(x, w).to(DEV)
                xd, wd = x.to(DEV), w.to(DEV)
                what = f"gemm_skinny M={M} N={N} K={K} split={split} ({len(sl)} slices)"
                gp.assert_exact(ops.linear(xd, wd, split=split), ref, what, 256, 64)
                sk = ops.linear(xd, wd, split=split, defer_reduce=True)
                if len(sl) == 1:
                    gp.assert_exact(sk, ref, what + " deferred (one slice)", 256, 64)
                else:
                    assert isinstance(sk, ops.SplitK) and sk.split == len(sl) and not sk.is_bf16, what
                    for s in range(len(sl)):
                        gp.assert_exact(sk.P[s], slabs[s], f"{what} deferred, slab {s}", 256, 64)
            # cfg: 0 = the register-ring GEMV (M <= 8), else the staged kernel's 16-row tiles
            COMBOS.add(("skinny", 0 if M <= 8 else (M + 15) // 16, (sl[-1][1] - sl[-1][0]) // 64, len(sl), "bf16+p32"))


@pytest.mark.parametrize("split", gp.ROWS_SPLITS)
@pytest.mark.parametrize("rw", gp.ROWS_RWS)
def test_gemv_rows_exact(rw, split):
    """linear_rows at its smallest K (512 per slice), N = 1, 3 and one past a workgroup's 4 rw rows, every
    staged row count (1, 2, 4, 8, 16), plain and deferred.  M * N is odd in many of these: the reduce
    kernel's scalar variant."""
    K = 512 * split
    sl = gp.even_slices(K, split)
    for N in gp.rows_ns(rw):
        for M in gp.ROWS_MS:
            assert ops.rows_ok(M, K, split)
            for seed in gp.draw_seeds(M, N, K, 16, 4 * rw):
                x, w = gp.make_xw(M, N, K, seed)
                slabs, ref = gp.want_slabs(x, w, sl).to(DEV), gp.want(x, w).to(DEV)
                xd, wd = x.to(DEV), w.to(DEV)
                what = f"gemv_rows M={M} N={N} K={K} split={split} rw={rw}"
                gp.assert_exact(ops.linear_rows(xd, wd, split, rw), ref, what, 16, 4 * rw)
                sk = ops.linear_rows(xd, wd, split, rw, defer_reduce=True)
                if split == 1:
                    gp.assert_exact(sk, ref, what + " deferred (one slice)", 16, 4 * rw)
                else:
                    assert isinstance(sk, ops.SplitK) and sk.split == split, what
                    for s in range(split):
                        gp.assert_exact(sk.P[s], slabs[s], f"{what} deferred, slab {s}", 16, 4 * rw)
            COMBOS.add(("rows", ops.rows_mr(M), rw, split, "bf16+p32"))


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("I", [1792, 2048])
def test_swiglu_linear_fused_is_exact(I, M):
    """swiglu_linear at the TP = 8 shard I = 1792 (fails rows_ok: ka_gemv_swiglu) and at 2048 (the row
    GEMV), gu small integers: bit-identical to silu_mul then the same GEMV (the activation is rounded
    to bf16 in both, so the integer-exact claim does not hold here)."""
    N = 520
    g = torch.Generator().manual_seed(I + M)
    gu = torch.randint(-4, 5, (M, 2 * I), generator=g).to(BF).to(DEV)
    w = gp.make_w(N, I, 9).to(DEV)
    rows = ops.ROWS_SWIGLU and ops.rows_ok(M, I, ops.ROWS_SWIGLU_SPLIT)
    assert rows == (I == 2048)
    got = ops.swiglu_linear(gu, w)
    if rows:
        want = ops.linear_rows(ops.silu_mul(gu), w, ops.ROWS_SWIGLU_SPLIT, ops.ROWS_SWIGLU_RW)
    else:
        want = ops.linear(ops.silu_mul(gu), w, split=ops.skinny_split(M, N, I, 256))
    assert torch.equal(got, want)
    parts = ops.swiglu_linear(gu, w, defer_reduce=True)
    if isinstance(parts, ops.SplitK):        # the reduce kernel's order: slice by slice
        acc = parts.P[0].clone()
        for k in range(1, parts.split):
            acc += parts.P[k]
        assert torch.equal(acc.to(BF), want)
    else:
        assert torch.equal(parts, want)
    COMBOS.add(("rows_swiglu" if rows else "gemv_swiglu", M, I // 64, 0, "bf16+p32"))
