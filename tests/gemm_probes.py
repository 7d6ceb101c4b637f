"""GEMM inputs with exact answers, their comparators, and a tiled reference GEMM that can be broken on
purpose (tests/test_gemm_probes_cpu.py proves that each probe rejects each break;
tests/test_gemm_probes_gpu.py runs the probes against csrc/gemm_mfma.hip, gemm_big.hip and
gemm_skinny.hip).  Importable without a GPU.

Integer family.  x holds +-1 in every position, so every row of every m-tile contributes at every k.
w holds {-1, 0, 1}: dense up to K = 2048 (the row GEMV's tiles are single columns, and its largest K
is 2048), about 1024 non-zeros per row above that, plus one forced non-zero per (k, 16-row group of
w), so every k contributes to every 16-column group of the output: losing a single k element of any
tile changes whole rows of that tile by +-1.  Products and partial sums are integers far below 2^24,
so fp32 accumulation is exact in any order, split and MFMA shape.  The variance of an output element
is at most 2048 (sd <= 46; 1024 + K / 16 above K = 2048), and the condition max |want| <= 256 (every
integer up to 256 is a bf16 value, so bf16 outputs and bf16 split-K slabs are exact too) is asserted
on the fp64 reference, never measured on a kernel: `want` and `want_slabs` raise if an input set
breaks it.

SwiGLU family.  Gate rows have 16 non-zeros (one per K / 16 stretch), so the gate pre-activation g is
an integer with |g| <= 16; up rows are the integer family.  The reference is silu(g) * u in fp64,
rounded once to bf16 (`round_bf16`); the kernels' fp32 g / (1 + __expf(-g)) * u may land on the other
side of a bf16 rounding boundary, so the comparator allows one bf16 ulp and demands an exact zero
where the reference is zero.

Argmax.  The LM head's rows repeat with period V / 2 - 8, so every integer logit of a row occurs two
or three times and the maximum ties across tiles, waves and lanes; mask row 0 repeats with the same
period (its rows always keep a tie), mask row 1 is random (the lower copy of a tie is often masked).
The expected index is the lowest allowed global token id among a row's maxima, from the exact logits
and the mask bits.
"""
from __future__ import annotations

import functools

import torch

BF = torch.bfloat16
BOUND = 256          # largest |integer| the probes allow in an output or a split-K slab
GATE_BOUND = 16
SENTINEL = 7.0
PAD_ROWS, PAD_COLS = 3, 8      # sentinel frame: rows above / below, columns left / right

# csrc/gemm_mfma.hip configurations: (BN weight rows, BM activation rows) and TN (16-row weight
# fragments per wave; the SwiGLU epilogue needs an even TN).  The GPU module checks this table against
# ka_gm_bn / ka_gm_bm.
GM_TILES = {2: (128, 256), 3: (256, 128), 4: (128, 128), 5: (128, 64), 6: (96, 256), 8: (192, 128),
            12: (128, 128), 19: (256, 256)}
GM_TN = {2: 4, 3: 4, 4: 4, 5: 4, 6: 3, 8: 6, 12: 4, 19: 8}
GM_ALL_CFGS = (2, 3, 4, 5, 6, 8, 12, 19)
GM_NKS = (1, 2, 3, 5, 7)       # k-steps of 64 per split-K slice
GM_SPLITS = (1, 2, 4)
GM_TP_SHAPES = ((128, 4096, 1792, 4), (16, 8192, 3584, 8))   # (M, N, K, split): nk = 7 in production


def gm_rows(cfg: int):
    bm = GM_TILES[cfg][1]
    return (1, bm - 1, bm + 1)


def gm_cols(cfg: int):
    return (16, GM_TILES[cfg][0] + 16)


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _signs(shape, g) -> torch.Tensor:
    return (torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1).float()


def w_density(K: int) -> float:
    return 1.0 if K <= 2048 else 1024.0 / K


def make_w(N: int, K: int, seed: int) -> torch.Tensor:
    """[N, K] bf16 in {-1, 0, 1} with a non-zero in every (k, 16-row group)."""
    g = _gen(seed)
    w = _signs((N, K), g)
    d = w_density(K)
    if d < 1.0:
        w = w * (torch.rand((N, K), generator=g) < d).float()
    k = torch.arange(K)
    forced = _signs((K,), g)
    for n0 in range(0, N, 16):
        r = min(16, N - n0)
        w[n0 + k % r, k] = forced
    return w.to(BF)


def make_x(M: int, K: int, seed: int) -> torch.Tensor:
    return _signs((M, K), _gen(seed + 7919)).to(BF)


@functools.lru_cache(maxsize=4)
def make_xw(M: int, N: int, K: int, seed: int = 0):
    """(x, w) of the integer family on the CPU; cached, so callers leave them unchanged."""
    return make_x(M, K, seed), make_w(N, K, seed)


def draw_seeds(M: int, N: int, K: int, bm: int, bn: int):
    """Seeds of the input sets a shape is probed with: one, or as many as give the last (ragged) output
    tile at least 8 elements in all (a single output element hides, say, two swapped k-chunks whenever
    the two sums happen to agree)."""
    last = (M - (M - 1) // bm * bm) * (N - (N - 1) // bn * bn)
    return [case_seed(M, N, K, d) for d in range(max(1, -(-8 // last)))]


def even_slices(K: int, split: int):
    kps = K // split
    return [(s * kps, (s + 1) * kps) for s in range(split)]


def skinny_slices(K: int, split: int):
    """csrc/gemm_skinny.hip's slices: 64-aligned, the last one may be shorter (and the split smaller)."""
    kps = ((K // split + 63) // 64) * 64
    return [(a, min(K, a + kps)) for a in range(0, K, kps)]


def _bounded(t: torch.Tensor, bound: int, what: str) -> torch.Tensor:
    m = float(t.abs().max()) if t.numel() else 0.0
    if m > bound:
        raise ValueError(f"probe inputs break the exactness condition: max |{what}| = {m} > {bound}")
    return t


def want(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x @ w.T in fp64 (on x's device), with the exactness condition asserted."""
    return _bounded(x.double() @ w.double().t(), BOUND, "want")


def want_slabs(x: torch.Tensor, w: torch.Tensor, slices) -> torch.Tensor:
    """[len(slices), M, N] fp64 split-K slabs, every one within the condition."""
    xd, wd = x.double(), w.double()
    return _bounded(torch.stack([xd[:, a:b] @ wd[:, a:b].t() for a, b in slices]), BOUND, "slab")


def _report(bad: torch.Tensor, got: torch.Tensor, ref: torch.Tensor, bm: int, bn: int) -> str:
    idx = bad.nonzero()
    first = [(int(r), int(c), float(got[r, c]), float(ref[r, c])) for r, c in idx[:6].tolist()]
    r0, r1 = int(idx[:, 0].min()), int(idx[:, 0].max())
    c0, c1 = int(idx[:, 1].min()), int(idx[:, 1].max())
    return (f"{idx.shape[0]} of {bad.numel()} elements wrong; first (row, col, got, want): {first}; "
            f"rows {r0}..{r1}, cols {c0}..{c1} = m-tiles {r0 // bm}..{r1 // bm}, n-tiles {c0 // bn}..{c1 // bn} "
            f"of {bm} x {bn} tiles")


def assert_exact(got: torch.Tensor, ref: torch.Tensor, what: str, bm: int = 256, bn: int = 256) -> None:
    """got (bf16 / fp32, any device) equals the fp64 reference element for element; no tolerance."""
    ref = ref.to(got.device)
    g = got.double()
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    if torch.equal(g, ref):
        return
    g, ref = g.cpu(), ref.cpu()
    raise AssertionError(f"{what}: {_report(g != ref, g, ref, bm, bn)}")


def assert_slabs_exact(P: torch.Tensor, ref: torch.Tensor, what: str, bm: int = 256, bn: int = 256) -> None:
    """Deferred fp32 or bf16 split-K slabs: P.float().sum(0) equals the reference exactly."""
    assert_exact(P.float().sum(0), ref, what + " (sum of slabs)", bm, bn)


# ---- the shapes the GPU module runs (tests/test_gemm_probes_cpu.py walks the same lists) ------------
BIG_KS, BIG_MS, BIG_NS = (128, 256, 384, 640), (1, 255, 257, 600), (128, 192, 384, 640)
BIG_SWIGLU_IS = (128, 384, 640)          # 2I % 256 == 0; I = 192 must be refused
# (M, N) at which gemm_big's choose_tn picks the 192-wide tile (TN 6) on 256 CUs: the smallest multiple
# of 384 per row count.  A partial round of 192-wide tiles costs 0.78 of a round, one of t 256-wide tiles
# 0.5 + 0.65 t / 256, so TN 6 wins from t = 111 tiles up: 111 tile columns for one tile row (M <= 256),
# 56 for two, 38 for three.  At the N of BIG_NS (t <= 9) the 256-wide tile always wins.
BIG_TN6_SHAPES = ((1, 28416), (255, 28416), (257, 14208), (600, 9600))
SKINNY_NS, SKINNY_KS, SKINNY_SPLITS, SKINNY_MS = (8, 60, 68), (64, 448, 4096), (1, 2, 3, 8), (1, 5, 64, 256)
ROWS_MS, ROWS_RWS, ROWS_SPLITS = (1, 2, 3, 5, 9, 16), (1, 2, 4, 8), (1, 2, 4)
ARGMAX_MS, ARGMAX_VK, ARGMAX_OFFS = (1, 7, 64, 257), ((128, 128), (640, 384), (64128, 256)), (0, 64128)


def rows_ns(rw: int):
    return (1, 3, rw * 4 + 1)


def gemm_cases():
    """(kernel, M, N, K, slices, bm, bn) of every integer-family GEMM shape of the GPU module, once per
    distinct tile geometry (cfg 4 and 12 share theirs).  gemm_big's split-tail slices are planned at run
    time from the CU count; the finest split they can be (one trip of 128 per slice) stands for them."""
    seen, out = set(), []

    def add(kernel, M, N, K, slices, bm, bn):
        key = (M, N, K, tuple(slices), bm, bn)
        if key not in seen:
            seen.add(key)
            out.append((kernel, M, N, K, slices, bm, bn))

    for cfg in GM_ALL_CFGS:
        bn, bm = GM_TILES[cfg]
        for nk in GM_NKS:
            for split in GM_SPLITS:
                K = 64 * nk * split
                for M in gm_rows(cfg):
                    for N in gm_cols(cfg):
                        add("gm", M, N, K, even_slices(K, split), bm, bn)
        for (M, N, K, split) in GM_TP_SHAPES:
            add("gm", M, N, K, even_slices(K, split), bm, bn)
    for K in BIG_KS:
        for M in BIG_MS:
            for N in BIG_NS:
                for bn in ((256, 192) if N % 192 == 0 else (256,)):
                    add("big", M, N, K, even_slices(K, 1), 256, bn)
                    if K > 128 and bn == 256:   # the split tail at its finest: one 128-deep trip per slice
                        add("big", M, N, K, even_slices(K, K // 128), 256, bn)
        for (M, N) in BIG_TN6_SHAPES:
            add("big", M, N, K, even_slices(K, 1), 256, 192)
    for N in SKINNY_NS:
        for K in SKINNY_KS:
            for split in SKINNY_SPLITS:
                for M in SKINNY_MS:
                    add("skinny", M, N, K, skinny_slices(K, split), 256, 64)
    for split in ROWS_SPLITS:
        for rw in ROWS_RWS:
            for N in rows_ns(rw):
                for M in ROWS_MS:
                    add("rows", M, N, 512 * split, even_slices(512 * split, split), 16, 4 * rw)
    out.sort(key=lambda c: (c[0], c[3], c[1], c[2], len(c[4])))   # equal inputs next to each other
    return out


def case_seed(*key) -> int:
    """A seed per case from plain integer arithmetic, the same on every interpreter."""
    h = 0x2545F491
    for k in key:
        h = (h * 1000003 + int(k) + 0x7F4A7C15) % (2 ** 31 - 1)
    return h


# ---- sentinels and strided operands ----------------------------------------------------------------
def framed_out(M: int, N: int, device, dtype=BF):
    """(whole, view): `whole` is filled with SENTINEL, `view` its [M, N] interior (row stride N + 16)."""
    whole = torch.full((M + 2 * PAD_ROWS, N + 2 * PAD_COLS), SENTINEL, dtype=dtype, device=device)
    return whole, whole[PAD_ROWS:PAD_ROWS + M, PAD_COLS:PAD_COLS + N]


def assert_frame_intact(whole: torch.Tensor, what: str) -> None:
    M, N = whole.shape[0] - 2 * PAD_ROWS, whole.shape[1] - 2 * PAD_COLS
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[PAD_ROWS:PAD_ROWS + M, PAD_COLS:PAD_COLS + N] = False
    bad = outside & (whole != SENTINEL)
    if bool(bad.any()):
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {idx.shape[0]} elements outside the out= view were written, first "
                             f"(row, col) relative to the view: "
                             f"{[(r - PAD_ROWS, c - PAD_COLS) for r, c in idx[:6].tolist()]}")


def strided(x: torch.Tensor) -> torch.Tensor:
    """x as a column slice of a tensor 8 columns wider (row stride K + 8, 16-B aligned start); the
    columns outside hold 3.0, which no probe input holds."""
    M, K = x.shape
    wide = torch.full((M, K + 8), 3.0, dtype=x.dtype, device=x.device)
    wide[:, 8:] = x
    v = wide[:, 8:]
    assert v.stride(0) == K + 8 and v.stride(1) == 1
    return v


# ---- SwiGLU ----------------------------------------------------------------------------------------
def make_gate(I: int, K: int, seed: int) -> torch.Tensor:
    """[I, K] bf16 gate rows with exactly one +-1 in each of the 16 stretches of K / 16 columns."""
    assert K % 16 == 0
    g = _gen(seed + 104729)
    st = K // 16
    pos = torch.arange(16) * st + torch.randint(0, st, (I, 16), generator=g)
    w = torch.zeros(I, K)
    w.scatter_(1, pos, _signs((I, 16), g))
    return w.to(BF)


def make_swiglu(M: int, I: int, K: int, seed: int = 0):
    """x [M, K] and w13 = [gate; up] ([2I, K], the model's layout)."""
    return make_x(M, K, seed), torch.cat([make_gate(I, K, seed), make_w(I, K, seed)], 0)


def round_bf16(v: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (ties to even) in ONE rounding, returned as bf16 (torch's own
    fp64 -> bf16 conversion rounds to fp32 first).  Integer arithmetic on the fp64 bit pattern: keep 7
    of the 52 mantissa bits.  Normal, finite values inside bf16's range only."""
    b = v.double().contiguous().view(torch.int64)
    b = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    return b.view(torch.float64).to(BF)


def want_swiglu(x: torch.Tensor, w13: torch.Tensor) -> torch.Tensor:
    I = w13.shape[0] // 2
    xd = x.double()
    g = _bounded(xd @ w13[:I].double().t(), GATE_BOUND, "gate")
    u = _bounded(xd @ w13[I:].double().t(), BOUND, "up")
    return round_bf16(g / (1.0 + torch.exp(-g)) * u)


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> int32 that orders like the values (both zeros -> 0); adjacent values differ by 1."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def assert_swiglu(got: torch.Tensor, ref: torch.Tensor, what: str, bm: int = 256, bn: int = 256):
    """At most one bf16 ulp per element, exact zeros where the reference is zero.  Returns (elements
    one ulp off, elements)."""
    assert got.dtype == BF and ref.dtype == BF and got.shape == ref.shape, what
    ref = ref.to(got.device)
    d = (_ordered(got) - _ordered(ref)).abs()
    bad = (d > 1) | ((ref == 0) & (got != 0)) | ~torch.isfinite(got.float())
    if bool(bad.any()):
        raise AssertionError(f"{what}: {_report(bad.cpu(), got.double().cpu(), ref.double().cpu(), bm, bn)}")
    return int((d == 1).sum()), d.numel()


# ---- argmax ----------------------------------------------------------------------------------------
def make_argmax_xw(M: int, V: int, K: int, seed: int = 0):
    """Integer-family x and an LM head whose rows repeat with period V / 2 - 8, so every logit of a row
    occurs two or three times, 8 short of half the vocabulary apart: the row's maximum ties across
    256-token tiles, across the two 128-column waves of a tile and across lanes."""
    period = argmax_period(V)
    return make_x(M, K, seed), make_w(period, K, seed)[torch.arange(V) % period].contiguous()


def argmax_period(V: int) -> int:
    return V // 2 - 8


def make_mask(V: int, off: int, seed: int = 1) -> torch.Tensor:
    """[2, ceil((V + off) / 32)] int32 mask words indexed by the global token id.  Row 1 is random, so
    the lower copy of a tied maximum is often masked and a higher one must win; row 0 repeats with the
    LM head's period inside the shard's ids [off, off + V), so the copies of a logit share their bit and
    every row that uses it has a tie among its allowed maxima."""
    import numpy as np
    words = (V + off + 31) // 32
    rs = np.random.RandomState(seed)
    flat = rs.randint(0, 2, size=(2, words * 32)).astype(np.uint64)
    period = argmax_period(V)
    flat[0, off:off + V] = flat[0, off:off + period][np.arange(V) % period]
    bits = (flat.reshape(2, words, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    return torch.from_numpy(bits.astype(np.uint32).view(np.int32))


def allowed_tokens(bits: torch.Tensor, midx: torch.Tensor, V: int, off: int) -> torch.Tensor:
    import numpy as np
    b = bits.cpu().numpy().view(np.uint32)
    gid = np.arange(V) + off
    out = torch.ones(midx.shape[0], V, dtype=torch.bool)
    for r, mi in enumerate(midx.tolist()):
        if mi >= 0:
            out[r] = torch.from_numpy(((b[mi][gid >> 5] >> (gid & 31)) & 1).astype(bool))
    return out


def expected_argmax(logits: torch.Tensor, allowed, off: int):
    """(global token id int32 [M], value fp32 [M]): the lowest allowed id among each row's maxima."""
    lg = logits.clone()
    if allowed is not None:
        lg = lg.masked_fill(~allowed, float("-inf"))
    best = lg.max(1).values
    assert bool(torch.isfinite(best).all()), "a probe row allows no token"
    first = (lg == best[:, None]).int().argmax(1)     # the first maximum
    return (first + off).to(torch.int32), best.float()


def pick_argmax(logits: torch.Tensor, allowed, off: int, tie: str = "lowest"):
    """A plain argmax over the exact logits; tie = "highest" is the mutation."""
    lg = logits if allowed is None else logits.masked_fill(~allowed, float("-inf"))
    best = lg.max(1).values
    hit = (lg == best[:, None]).int()
    V = lg.shape[1]
    idx = hit.argmax(1) if tie == "lowest" else V - 1 - hit.flip(1).argmax(1)
    return (idx + off).to(torch.int32), best.float()


def assert_argmax(idx, val, want_idx, want_val, what: str) -> None:
    idx, val = idx.cpu(), val.cpu().float()
    want_idx, want_val = want_idx.cpu(), want_val.cpu()
    bad = ((idx != want_idx) | (val != want_val)).nonzero().flatten().tolist()
    assert not bad, (f"{what}: {len(bad)} of {idx.numel()} rows wrong; first (row, idx, want idx, val, want val): "
                     f"{[(r, int(idx[r]), int(want_idx[r]), float(val[r]), float(want_val[r])) for r in bad[:6]]}")


# ---- the tiled reference with injectable mutations -------------------------------------------------
MUTATIONS = ("drop_k", "drop_step", "double_step", "stale_step", "swap_chunk", "lose_slice", "double_slice",
             "row_shift")


def mutation_applies(mut: str, M: int, slices) -> bool:
    """stale_step needs a step before the last one; a lost or doubled slice needs split-K; a row index
    shifted by one (modulo M, as the kernels wrap rows) is the identity with a single row."""
    if mut == "stale_step":
        return slices[-1][1] - slices[-1][0] >= 128
    if mut in ("lose_slice", "double_slice"):
        return len(slices) > 1
    if mut == "row_shift":
        return M > 1
    return True


def tiled_gemm(x: torch.Tensor, w: torch.Tensor, bm: int, bn: int, slices, mut=None, kk: int = 37,
               base=None) -> torch.Tensor:
    """fp32 split-K slabs [len(slices), M, N] of x @ w.T computed as a tiled kernel does: bm x bn
    output tiles, 64-deep k-steps, fp32 accumulation.  Every tile but the last (m-tile, n-tile) of the
    last slice is one matmul; that tile is accumulated step by step, and `mut` breaks it there:
      drop_k        the last k-step loses element kk of its 64
      drop_step / double_step   the last k-step is skipped / added twice
      stale_step    the last k-step re-reads the operands of the step before
      swap_chunk    in the last k-step X's 8-element chunk c meets W's chunk c ^ 1
      lose_slice / double_slice the tile's last split-K slice is zero / counted twice
      row_shift     the rows of the last m-tile read X row (m + 1) % M
    base: the unmutated slabs of the same call, to skip recomputing the untouched tiles."""
    assert mut is None or mut in MUTATIONS
    M, N = x.shape[0], w.shape[0]
    if base is not None:
        P = base.clone()
    else:
        xf, wf = x.float(), w.float()
        P = torch.stack([xf[:, a:b] @ wf[:, a:b].t() for a, b in slices])
    m0, n0 = (M - 1) // bm * bm, (N - 1) // bn * bn
    a, b = slices[-1]
    rows = torch.arange(m0, M)
    if mut == "row_shift":
        rows = (rows + 1) % M
    xt, wt = x[rows][:, a:b].float(), w[n0:N, a:b].float()
    steps = (b - a) // 64
    acc = torch.zeros(M - m0, N - n0)
    for t in range(steps):
        last = t == steps - 1
        src = t - 1 if (last and mut == "stale_step") else t
        xs, ws = xt[:, src * 64:(src + 1) * 64], wt[:, src * 64:(src + 1) * 64]
        if last and mut == "swap_chunk":
            xs = xs.reshape(-1, 4, 2, 8).flip(2).reshape(-1, 64)
        if last and mut == "drop_k":
            xs = xs.clone()
            xs[:, kk] = 0
        c = xs @ ws.t()
        if last and mut == "drop_step":
            continue
        acc += 2 * c if (last and mut == "double_step") else c
    if mut == "lose_slice":
        acc.zero_()
    elif mut == "double_slice":
        acc *= 2
    P[-1, m0:, n0:] = acc
    return P


def swiglu_from_gu(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The kernels' epilogue on exact fp32 accumulators, in fp32 as they compute it."""
    g, u = g.float(), u.float()
    return (g / (1.0 + torch.exp(-g)) * u).to(BF)
