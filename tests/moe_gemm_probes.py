"""Exact probes for the two kernels that do the MoE arithmetic: moe_gemm_kernel<MT> (csrc/moe.hip,
ka_moe_gemm: the decode-path expert GEMM over gathered rows, split-K) and gemm256_kernel<EPI, 8, GR>
(csrc/gemm_big.hip, ka_gemm_big_grouped: the prefill-path GEMM over expert-sorted rows and a chunk
table).  Inputs, fp64 references, comparators, and plain-torch emulators of both kernels that walk
chunks, tiles and workgroups the way the kernels do and can be broken on purpose
(tests/test_moe_gemm_probes_cpu.py proves that every probe rejects every break that applies to it;
tests/test_moe_gemm_probes_gpu.py runs the same case lists against the kernels).  Importable without
a GPU.

Inputs are gemm_probes' integer family (x rows of +-1, w in {-1, 0, 1}, gate rows with 16 non-zeros),
one weight seed per expert and distinct random sign rows, so a row gathered from the wrong source or
multiplied by the wrong expert's weights changes the answer; every output and split-K slab is an
integer within gemm_probes.BOUND, asserted on the fp64 reference (`want`), never on a kernel.

Where a break makes two tiles write one place (a race in a real kernel), it counts as applying to a
case only if it also writes a place no correct tile writes (a gap row, the decoy row, a Y row that no
out_rows entry names), so its rejection does not depend on which write lands last.
"""
from __future__ import annotations

import functools

import torch

from tests import elementwise_probes as ep
from tests import gemm_probes as gp
from tests.gemm_probes import BF, SENTINEL, case_seed

K_MUTATIONS = ("drop_k", "drop_step", "swap_chunk")                 # gemm_probes' k-loop breaks, last tile
MOE_MUTATIONS = K_MUTATIONS + ("lose_slice", "double_slice", "wrong_expert", "stale_rows", "src_div_ignored",
                               "short_slice_full", "chunk_clamp", "row_clamp")
GROUPED_MUTATIONS = K_MUTATIONS + ("wrong_expert", "stale_rows", "hole_consumed", "skip_after_hole", "wrap_stored",
                                   "sorted_not_slot", "gate_up_swap")
MUTATIONS = tuple(dict.fromkeys(MOE_MUTATIONS + GROUPED_MUTATIONS))


def _flat_rows(mat: torch.Tensor, rows: torch.Tensor, k0: int, k1: int) -> torch.Tensor:
    """mat[rows, k0:k1] read as the kernels address memory: row * K + k into the flat array, so a k past
    the row's end (a break that reads too far) runs into the next row; wrapped at the array's end."""
    K = mat.shape[-1]
    flat = mat.reshape(-1)
    idx = (rows.long()[:, None] * K + torch.arange(k0, k1)[None, :]) % flat.numel()
    return flat[idx].float()


def _k_loop(xt: torch.Tensor, wt: torch.Tensor, mut, kk: int) -> torch.Tensor:
    """xt @ wt.T in 64-deep steps with one of gemm_probes.tiled_gemm's breaks in the last step."""
    steps = xt.shape[1] // 64
    acc = torch.zeros(xt.shape[0], wt.shape[0])
    for t in range(steps):
        xs, ws = xt[:, 64 * t:64 * t + 64], wt[:, 64 * t:64 * t + 64]
        if t == steps - 1:
            if mut == "drop_step":
                continue
            if mut == "swap_chunk":
                xs = xs.reshape(-1, 4, 2, 8).flip(2).reshape(-1, 64)
            if mut == "drop_k":
                xs = xs.clone()
                xs[:, kk] = 0
        acc += xs @ ws.t()
    return acc


# ====================================================================================================
# ka_moe_gemm
# ====================================================================================================
MOE_MAX_ROWS = (2, 16, 17, 33, 64, 65, 128, 129, 300)
MOE_KS = ((64, 1), (128, 1), (192, 1), (320, 1), (320, 2), (448, 3), (512, 4))      # (K, split)
MOE_NS = (4, 60, 64, 68, 132)
MOE_SRC_DIVS = (1, 2)
# max_rows -> per-expert row counts (one of them per case, in turn).  MT = 1, 1, 2, 4, 4, 8, 8, 8, 8 and
# with MT = 8 one, two and three row chunks.  Counts hold 0, 1, counts that are no multiple of 16,
# exactly MT * 16 (16, 64, 128) and MT * 16 + 1 (129; 257 = 2 MT * 16 + 1).  Where the counts leave no
# row over (16, 64, 128 rows on one expert) there is no decoy row and no list entry past a count is ever
# inside a tile's reach; everywhere else the rows left over belong to no expert and the first is the decoy.
MOE_COUNTS = {
    2: ((0, 1),),
    16: ((16, 0), (0, 1, 7, 5, 2)),
    17: ((0, 1, 5, 10),),
    33: ((0, 1, 20, 11),),
    64: ((64, 0), (0, 33, 1, 16, 13)),
    65: ((0, 1, 37, 26),),
    128: ((128, 0), (0, 1, 100, 26)),
    129: ((128, 0),),
    300: ((257, 0, 1, 41), (129, 0, 128, 1, 41)),
}
# ka_moe_gemm must refuse these (K, N, split, with P): K % 64, N % 4, split < 1, split > 1 without P, an
# empty last slice (K = 256 at split 3: slices of 128, 128 and none)
MOE_REFUSED = ((96, 64, 1, False), (128, 6, 1, False), (128, 64, 0, False), (128, 64, 2, False), (256, 64, 3, True))


def moe_mt(max_rows: int) -> int:
    mt = (max_rows + 15) // 16
    return 1 if mt <= 1 else 2 if mt <= 2 else 4 if mt <= 4 else 8


def moe_kps(K: int, split: int) -> int:
    return (K // 64 + split - 1) // split * 64


def moe_slices(K: int, split: int):
    kps = moe_kps(K, split)
    assert (K + kps - 1) // kps == split, "a slice would be empty"
    return [(s * kps, min(K, (s + 1) * kps)) for s in range(split)]


def moe_cases():
    """(max_rows, counts, K, split, N, src_div): every max_rows with every (K, split); N and src_div in
    turn, so every MT and every (K, split) meets every N and both row sources."""
    out = []
    for i, mr in enumerate(MOE_MAX_ROWS):
        for j, (K, split) in enumerate(MOE_KS):
            cs = MOE_COUNTS[mr]
            out.append((mr, cs[j % len(cs)], K, split, MOE_NS[(i + j) % len(MOE_NS)], MOE_SRC_DIVS[(i + j) % 2]))
    return out


@functools.lru_cache(maxsize=4)
def moe_inputs(case):
    """(A [ceil(max_rows / src_div), K], W [el, N, K], counts int32 [el], lists int32 [el, max_rows], decoy).
    Expert e's rows are a stretch of a fixed shuffle of range(max_rows); list entries past a count hold
    the decoy row (a valid row of no expert), or row 0 where no row is left over.  Cached: read-only."""
    mr, cs, K, split, N, sd = case
    seed = case_seed(mr, K, split, N, sd)
    A = gp.make_x((mr + sd - 1) // sd, K, seed)
    W = torch.stack([gp.make_w(N, K, seed + 1 + e) for e in range(len(cs))])
    perm = torch.randperm(mr, generator=gp._gen(seed)).int()
    used = sum(cs)
    assert used <= mr
    decoy = int(perm[used]) if used < mr else None
    lists = torch.full((len(cs), mr), 0 if decoy is None else decoy, dtype=torch.int32)
    o = 0
    for e, c in enumerate(cs):
        lists[e, :c] = perm[o:o + c]
        o += c
    return A, W, torch.tensor(cs, dtype=torch.int32), lists, decoy


def moe_want(case, inp, device="cpu") -> torch.Tensor:
    """fp64 [split, max_rows, N]: slab s holds expert e's product over slice s on e's listed rows and the
    sentinel on every other row (the decoy included).  split == 1: [1, ..] is Y."""
    mr, cs, K, split, N, sd = case
    A, W, counts, lists, _ = inp
    A, W = A.to(device), W.to(device)
    sl = moe_slices(K, split)
    out = torch.full((split, mr, N), SENTINEL, dtype=torch.float64, device=device)
    for e, c in enumerate(cs):
        if c:
            rows = lists[e, :c].long().to(device)
            x = A[rows // sd]
            gp.want(x, W[e])                                       # the whole product within the bound too
            out[:, rows] = gp.want_slabs(x, W[e], sl)
    return out


def assert_moe(got: torch.Tensor, ref: torch.Tensor, what: str, rows: int = 16) -> None:
    """Y bf16 [max_rows, N] or P fp32 [split, max_rows, N] against moe_want, element for element, the
    sentinels of unlisted rows included."""
    N = ref.shape[-1]
    gp.assert_exact(got.reshape(-1, N), ref.reshape(-1, N), what, rows, 64)


def _moe_tiles(case):
    """(expert, row chunk, slice, column tile) of every workgroup that passes `r0 >= count`, in grid order."""
    mr, cs, K, split, N, sd = case
    ROWS = 16 * moe_mt(mr)
    return [(e, rc, ks, nt) for e, c in enumerate(cs) for rc in range((mr + ROWS - 1) // ROWS) if rc * ROWS < c
            for ks in range(split) for nt in range((N + 63) // 64)]


def moe_target(mut: str, case, inp):
    """The tile `mut` breaks: the last one it can change, or None where it cannot apply to the case."""
    mr, cs, K, split, N, sd = case
    A, _, _, lists, decoy = inp
    ROWS, kps = 16 * moe_mt(mr), moe_kps(K, split)
    busy = [e for e, c in enumerate(cs) if c]

    def ok(t):
        e, rc, ks, nt = t
        nrows = min(ROWS, cs[e] - rc * ROWS)
        nch = min(kps, K - ks * kps) // 64
        if mut in ("lose_slice", "double_slice"):
            return split > 1
        if mut == "wrong_expert":
            return e != busy[0]
        if mut == "stale_rows":
            return rc > 0
        if mut == "src_div_ignored":
            r = lists[e, rc * ROWS:rc * ROWS + nrows].long()
            return sd > 1 and bool((r % A.shape[0] != r // sd).any())
        if mut == "short_slice_full":
            return K - ks * kps < kps
        if mut == "chunk_clamp":
            return nch == 1
        if mut == "row_clamp":      # a list entry past the count inside the tile's reach, and it names the decoy
            return decoy is not None and nrows < ROWS and cs[e] < mr
        return True

    hits = [t for t in _moe_tiles(case) if ok(t)]
    return hits[-1] if hits else None


def moe_gemm_emulate(case, inp, mut=None, base=None, kk: int = 37) -> torch.Tensor:
    """fp32 [split, max_rows, N] (sentinel where nothing is stored) computed as moe_gemm_kernel<MT> does:
    workgroup (e, row chunk, slice, 64-column tile), nrows = min(ROWS, count - r0), source rows
    lists[e][r0 + i] / src_div, nchunks = min(kps, K - kb) / 64 chunks of 64, stores at lists[e][r0 + m] for
    m < nrows.  `mut` breaks the tile moe_target names:
      drop_k / drop_step / swap_chunk / lose_slice / double_slice   as gemm_probes.tiled_gemm
      wrong_expert      the weights of the expert before (the last one that had rows)
      stale_rows        the source rows of the row chunk before (stored at its own rows)
      src_div_ignored   row r of A instead of r / src_div
      short_slice_full  the short last slice reads a full kps of k
      chunk_clamp       a one-chunk slice also multiplies by the W chunk after it (load_w without its clamp)
      row_clamp         rows nrows .. ROWS - 1 (copies of row nrows - 1) are stored too, at the rows the
                        list names there
    base: the unbroken result of the same case; only the broken tile is recomputed."""
    mr, cs, K, split, N, sd = case
    A, W, _, lists, _ = inp
    ROWS, kps = 16 * moe_mt(mr), moe_kps(K, split)
    out = base.clone() if base is not None else torch.full((split, mr, N), SENTINEL)
    target = moe_target(mut, case, inp) if mut else None
    assert mut is None or target is not None, f"{mut} does not apply"
    lflat = lists.reshape(-1)
    busy = [e for e, c in enumerate(cs) if c]
    for tile in _moe_tiles(case):
        m = mut if tile == target else None
        if base is not None and m is None:
            continue
        e, rc, ks, nt = tile
        r0 = rc * ROWS
        nrows = min(ROWS, cs[e] - r0)
        li = lflat[e * mr + r0 + torch.arange(nrows)].long()
        src = lflat[e * mr + r0 - ROWS + torch.arange(nrows)].long() if m == "stale_rows" else li
        src = src % A.shape[0] if m == "src_div_ignored" else src // sd
        kb = ks * kps
        k1 = kb + (kps if m == "short_slice_full" else min(kps, K - kb))
        n0, n1 = 64 * nt, min(N, 64 * nt + 64)
        we = busy[busy.index(e) - 1] if m == "wrong_expert" else e
        wrows = we * N + torch.arange(n0, n1)
        xt, wt = _flat_rows(A, src, kb, k1), _flat_rows(W, wrows, kb, k1)
        acc = _k_loop(xt, wt, m, kk) if m in K_MUTATIONS else xt @ wt.t()
        if m == "chunk_clamp":
            acc = acc + xt @ _flat_rows(W, wrows, kb + 64, kb + 128).t()
        if m == "lose_slice":
            acc = torch.zeros_like(acc)
        if m == "double_slice":
            acc = 2 * acc
        out[ks, li, n0:n1] = acc
        if m == "row_clamp":
            extra = lflat[(e * mr + r0 + torch.arange(nrows, ROWS)) % lflat.numel()].long()
            out[ks, extra, n0:n1] = acc[nrows - 1]
    return out


def moe_combine_routing(case, inp):
    """(T, k, topk_ids int32 [T, k], topk_w fp32 [T, k]) that routes slot row r to the expert listing it,
    and every other row (the decoy included) to expert el, outside the window [0, el)."""
    mr, cs = case[0], case[1]
    k = 2 if mr % 2 == 0 else 1
    ids = torch.full((mr,), len(cs), dtype=torch.int32)
    for e, c in enumerate(cs):
        ids[inp[3][e, :c].long()] = e
    w = 2.0 ** torch.randint(-2, 1, (mr,), generator=gp._gen(case_seed(*case[2:], mr))).float()
    return mr // k, k, ids.view(-1, k), w.view(-1, k)


# ====================================================================================================
# ka_gemm_big_grouped
# ====================================================================================================
GROUPED_KS = (128, 256, 384)                   # 1, 2 and 3 trips of the k-loop
GROUPED_WIDTHS = {"bf16": (256, 2048), "swiglu": (128, 1024)}      # N / I
PERSISTENT_WIDTH = {"bf16": 2048, "swiglu": 1024}                   # 8 n-tiles either way
SORTED_R, SORTED_K = 1026, 256
# a chunk table written by hand: (expert, rows) of a chunk, an int g = a gap of g sorted rows that belong to
# no chunk, None = an unused (all-zero) entry.  Row counts 256, 1, 3, 17, 64, 255 and 1; expert 1 spans two
# chunks (256 + 1), expert 0 owns two separate small ones, expert 4 has none; gnr = 1, 3 and 255 re-read rows
# through row % gnr; sorted rows 0 and 1 are a gap (an unused entry run as expert 0 would write them) and so
# are the rows after the last chunk, whose gnr is 1 (rows stored past a count land there).
HAND_GROUPS = 6
HAND_TABLE = (None, 2, (1, 256), (1, 1), None, 3, (0, 3), (2, 17), (3, 64), None, 2, (5, 255), (0, 1), 3, None)
PERSIST_GROUPS = 4
PERSIST_ROWS = (1, 3, 17, 64, 2, 255, 9, 31, 256, 5)
PATTERNS = ("hole_then_tile", "tile_hole_tile", "tile_then_holes", "tiles_of_two_experts", "same_expert_two_chunks")


def xcd_logical(bid: int, nwg: int) -> int:
    """csrc/common.h xcd_logical."""
    xcd, q, r = bid & 7, nwg >> 3, nwg & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


def tile_of(L: int, tiles_m: int, tiles_n: int, gm: int = 8):
    """csrc/common.h tile_of."""
    per = gm * tiles_n
    g = L // per
    first = g * gm
    rows = min(gm, tiles_m - first)
    inn = L - g * per
    return first + inn % rows, inn // rows


def grouped_schedule(entries: int, tiles_n: int, cus: int):
    """[workgroup] -> [(entry, n-tile)] in the order launch_grouped's grid of min(tiles, cus) workgroups
    decodes its units (v = b, b + G, ..): holes included."""
    total = entries * tiles_n
    G = min(total, cus)
    assert G == total or G % 8 == 0
    return [[tile_of(xcd_logical(v, total), entries, tiles_n) for v in range(b, total, G)] for b in range(G)]


def grouped_patterns(tab, tiles_n: int, cus: int):
    """How many workgroups meet each of PATTERNS, and the most units / tiles one workgroup runs."""
    n = {p: 0 for p in PATTERNS}
    most_units = most_tiles = 0
    for seq in grouped_schedule(len(tab), tiles_n, cus):
        used = [tab[tm][2] > 0 for tm, _ in seq]
        tiles = [i for i, u in enumerate(used) if u]
        most_units, most_tiles = max(most_units, len(seq)), max(most_tiles, len(tiles))
        if not tiles:
            continue
        n["hole_then_tile"] += tiles[0] > 0
        n["tile_then_holes"] += tiles[-1] < len(seq) - 1
        for a, b in zip(tiles, tiles[1:]):
            ea, eb = tab[seq[a][0]], tab[seq[b][0]]
            n["tile_hole_tile"] += b > a + 1
            n["tiles_of_two_experts"] += b == a + 1 and ea[0] != eb[0]
            n["same_expert_two_chunks"] += b == a + 1 and ea[0] == eb[0] and seq[a][0] != seq[b][0]
    return n, most_units, most_tiles


def _layout(spec):
    """HAND_TABLE-style spec -> ([entries][4] table, sorted rows M)."""
    tab, r = [], 0
    for s in spec:
        if s is None:
            tab.append((0, 0, 0, 0))
        elif isinstance(s, int):
            r += s
        else:
            tab.append((s[0], r, s[1], 0))
            r += s[1]
    return tab, r


@functools.lru_cache(maxsize=8)
def persistent_spec(cus: int, tiles_n: int = 8):
    """The table for the persistent regime on `cus` workgroups: 4 cus / tiles_n + 8 entries, at least
    136 (more than 4 cus tiles: with 8 n-tiles and 64, 128 or 256 workgroups, consecutive units of a
    workgroup stay on one entry for up to half a super-row of 8 entries x 8 n-tiles, so it takes a fifth
    unit to see a third entry, which "tile, hole, tile" needs), unused entries at the start, in the middle, at the end and at random places between, the
    experts drawn at random (an expert owns several small chunks), a gap of 2 rows at the start and after
    every fifth chunk, 3 rows after the last chunk (whose gnr is 3).  The first draw in which the mirror of
    the launch (grouped_schedule) shows every one of PATTERNS on some workgroup."""
    entries = max(4 * cus // tiles_n + 8, 136)
    for attempt in range(64):
        g = gp._gen(case_seed(cus, tiles_n, attempt))
        hole = (torch.rand(entries, generator=g) < 0.35).tolist()
        experts = torch.randint(0, PERSIST_GROUPS, (entries,), generator=g).tolist()
        hole[0] = hole[entries // 2] = hole[-1] = True
        hole[1] = hole[-2] = False
        spec, used = [2], 0
        for i in range(entries):
            if hole[i]:
                spec.append(None)
                continue
            # sorted rows 0 .. must not be expert 0's (hole_consumed would write what is there already)
            spec.append((experts[i] or 1 if used == 0 else experts[i], 3 if i == entries - 2 else PERSIST_ROWS[used % 10]))
            used += 1
            if used % 5 == 0:
                spec.append(2)
        spec.append(3)
        tab, _ = _layout(spec)
        if all(grouped_patterns(tab, tiles_n, cus)[0].values()):
            return tuple(spec)
    raise AssertionError(f"no table with every workgroup pattern for {cus} workgroups, {tiles_n} n-tiles")


def grouped_cases(cus: int):
    """(table, epilogue, K, width) of every grouped probe: the hand-written single-pass table over every K
    and width, the table ka_moe_sort makes of elementwise_probes.MOE_ROUTINGS[1026], and the persistent
    table for `cus` workgroups over every K."""
    out = [("hand", epi, K, wd) for epi in ("bf16", "swiglu") for K in GROUPED_KS for wd in GROUPED_WIDTHS[epi]]
    out += [("sorted", epi, SORTED_K, PERSISTENT_WIDTH[epi]) for epi in ("bf16", "swiglu")]
    out += [("persistent", epi, K, PERSISTENT_WIDTH[epi]) for epi in ("bf16", "swiglu") for K in GROUPED_KS]
    return out


def tiles_n_of(epi: str, width: int) -> int:
    return width // 128 if epi == "swiglu" else width // 256


@functools.lru_cache(maxsize=16)
def _weights(epi: str, groups: int, width: int, K: int):
    if epi == "swiglu":     # [groups][gate rows; up rows][K]
        return torch.stack([torch.cat([gp.make_gate(width, K, 977 + e), gp.make_w(width, K, 977 + e)], 0)
                            for e in range(groups)])
    return torch.stack([gp.make_w(width, K, 977 + e) for e in range(groups)])


def sorted_routing():
    """(x [T, K], counts, lists, src_div, max_chunks) that ka_moe_sort turns into the "sorted" table."""
    T, k, cs = ep.MOE_ROUTINGS[SORTED_R]
    counts, lists = ep.moe_sort_lists(ep.moe_routing(SORTED_R), 0, len(cs))
    return gp.make_x(T, SORTED_K, 4242), counts, lists, k, (SORTED_R + 255) // 256 + len(cs)


@functools.lru_cache(maxsize=4)
def grouped_inputs(case, cus: int):
    """dict(X [M, K] sorted rows, W [groups, N or 2I, K], tab [[e, r0, rows, 0]], M, groups, out_rows int32 [M]
    (an injective map into Yrows > M rows; bf16 only) and Yrows).  Cached: read-only."""
    kind, epi, K, width = case
    if kind == "sorted":
        x, counts, lists, sd, chunks = sorted_routing()
        xs, slot, tab = ep.moe_sort_want(x, counts, lists, sd, chunks)
        d = dict(X=xs, tab=[tuple(t) for t in tab.tolist()], M=SORTED_R, groups=len(counts), out_rows=slot,
                 Yrows=SORTED_R)
        assert all(t == (0, 0, 0, 0) for t in d["tab"][8:]) and all(t[2] > 0 for t in d["tab"][:8])
    else:
        spec, groups = (HAND_TABLE, HAND_GROUPS) if kind == "hand" else (persistent_spec(cus), PERSIST_GROUPS)
        tab, M = _layout(spec)
        Yrows = M + 9
        perm = torch.randperm(Yrows, generator=gp._gen(case_seed(M, K))).int()
        d = dict(X=gp.make_x(M, K, case_seed(M, K, 1)), tab=tab, M=M, groups=groups, out_rows=perm[:M], Yrows=Yrows)
    d["W"] = _weights(epi, d["groups"], width, K)
    if epi == "swiglu":
        d["out_rows"], d["Yrows"] = None, d["M"]
    check_table(d["tab"], d["M"], d["groups"])
    return d


def check_table(tab, M: int, groups: int) -> None:
    """The kernel's contract: expert < groups, 1 <= rows <= 256, rows inside [0, M), chunks disjoint."""
    seen = torch.zeros(M, dtype=torch.bool)
    for (e, r0, n, z) in tab:
        if (e, r0, n, z) == (0, 0, 0, 0):
            continue
        assert 0 <= e < groups and 1 <= n <= 256 and 0 <= r0 and r0 + n <= M and z == 0, (e, r0, n)
        assert not bool(seen[r0:r0 + n].any()), "chunks overlap"
        seen[r0:r0 + n] = True


def grouped_want(case, d, device="cpu") -> torch.Tensor:
    """bf16: fp64 [Yrows, N], out_rows[r] = X[r] W[e]^T for every chunk row r and the sentinel elsewhere.
    SwiGLU: bf16 [M, I], sorted row r = round_bf16(silu(x gate^T) * (x up^T)), the sentinel on gap rows."""
    kind, epi, K, width = case
    X, W = d["X"].to(device), d["W"].to(device)
    out = torch.full((d["Yrows"], width), SENTINEL, dtype=BF if epi == "swiglu" else torch.float64, device=device)
    for (e, r0, n, _) in d["tab"]:
        if n == 0:
            continue
        if epi == "swiglu":
            out[r0:r0 + n] = gp.want_swiglu(X[r0:r0 + n], W[e])
        else:
            out[d["out_rows"][r0:r0 + n].long().to(device)] = gp.want(X[r0:r0 + n], W[e])
    return out


def chunk_rows(d) -> torch.Tensor:
    """bool [Yrows]: the output rows some chunk writes."""
    m = torch.zeros(d["Yrows"], dtype=torch.bool)
    for (e, r0, n, _) in d["tab"]:
        idx = torch.arange(r0, r0 + n)
        m[idx if d["out_rows"] is None else d["out_rows"][idx].long()] = True
    return m


def assert_grouped(case, d, got: torch.Tensor, ref: torch.Tensor, what: str):
    """bf16: exact, sentinels included.  SwiGLU: one bf16 ulp on chunk rows (an exact zero where the
    reference is zero), the sentinel bit for bit on every other row; returns (one ulp off, elements)."""
    if case[1] == "bf16":
        gp.assert_exact(got, ref, what, 256, 256)
        return 0, 0
    rows = chunk_rows(d).to(got.device)
    rest = got[~rows]
    assert bool((rest == SENTINEL).all()), f"{what}: {int((rest != SENTINEL).any(1).sum())} rows of no chunk were written"
    return gp.assert_swiglu(got[rows], ref.to(got.device)[rows], what + " (chunk rows, in order)", 256, 128)


def _last_tile(d, tiles_n: int):
    return max(i for i, t in enumerate(d["tab"]) if t[2] > 0), tiles_n - 1


def grouped_applies(mut: str, case, d, cus: int) -> bool:
    kind, epi, K, width = case
    tab, M = d["tab"], d["M"]
    tiles_n = tiles_n_of(epi, width)
    covered = torch.zeros(M + 256, dtype=torch.bool)
    for (e, r0, n, _) in tab:
        covered[r0:r0 + n] = True
    if mut in K_MUTATIONS:
        return True
    if mut == "gate_up_swap":
        return epi == "swiglu"
    if mut == "sorted_not_slot":
        return epi == "bf16" and any(int(d["out_rows"][r]) != r for (e, r0, n, _) in tab for r in range(r0, r0 + n))
    if mut == "hole_consumed":      # an unused entry, and a row of no chunk among sorted rows 0 .. 255
        return any(t[2] == 0 for t in tab) and not bool(covered[:min(256, M)].all())
    if mut == "wrap_stored":        # a chunk whose rows past its count reach a row of no chunk
        return any(n < 256 and not bool(covered[r0 + n:min(r0 + 256, M)].all()) for (e, r0, n, _) in tab if n)
    for seq in grouped_schedule(len(tab), tiles_n, cus):
        prev, hole = None, False
        for (tm, tn) in seq:
            t = tab[tm]
            if t[2] == 0:
                hole = True
                continue
            if mut == "skip_after_hole" and hole:
                return True
            if prev is not None and ((mut == "wrong_expert" and prev[0] != t[0]) or (mut == "stale_rows" and prev[1] != t[1])):
                return True
            prev, hole = t, False
    return False


def grouped_emulate(case, d, cus: int, mut=None, kk: int = 37) -> torch.Tensor:
    """The output of gemm256_kernel<EPI, 8, GR = true> computed the way the kernel walks: workgroup b of
    min(tiles, cus) takes units b, b + G, .. (grouped_schedule), skips unused entries, and for a tile
    (entry (ge, gr0, gnr), n-tile) stages X rows gr0 + row % gnr and expert ge's W rows, and stores rows
    below gnr at out_rows[gr0 + row] (bf16) or gr0 + row (SwiGLU).  Returns what the GPU test reads: bf16
    [Yrows, N] / [M, I] with the sentinel where nothing is stored.  `mut`:
      drop_k / drop_step / swap_chunk   the last tile, as gemm_probes.tiled_gemm
      wrong_expert     a tile uses the weights of the expert of the tile its workgroup ran before it
      stale_rows       a tile reads the rows of the chunk of the tile its workgroup ran before it
      hole_consumed    an unused entry runs as expert 0 on sorted rows 0 .. 255
      skip_after_hole  a tile whose workgroup skipped an unused entry just before it is lost
      wrap_stored      rows gnr .. 255 of a tile (copies of rows row % gnr) are stored too
      sorted_not_slot  bf16 stores land at the sorted row instead of out_rows[row]
      gate_up_swap     the last tile exchanges the gate and up halves of w13"""
    kind, epi, K, width = case
    X, W, tab, M, out_rows = d["X"], d["W"], d["tab"], d["M"], d["out_rows"]
    tiles_n = tiles_n_of(epi, width)
    bn = 128 if epi == "swiglu" else 256
    assert mut is None or grouped_applies(mut, case, d, cus), f"{mut} does not apply"
    out = torch.full((d["Yrows"], width), SENTINEL, dtype=BF)
    last = _last_tile(d, tiles_n)
    Xf = X.float()

    def run(ge, gr0, gnr, tn, we, xr0, m, nstore):
        rows = torch.arange(nstore)
        xr = (xr0 + rows % gnr) % M
        cols = torch.arange(bn * tn, bn * tn + bn)
        xt = Xf[xr]
        if epi == "swiglu":
            I = width
            g, u = W[we][cols].float(), W[we][I + cols].float()
            if m == "gate_up_swap":
                g, u = u, g
            gg = _k_loop(xt, g, m, kk) if m in K_MUTATIONS else xt @ g.t()
            uu = _k_loop(xt, u, m, kk) if m in K_MUTATIONS else xt @ u.t()
            val = gp.swiglu_from_gu(gg, uu)
        else:
            w = W[we][cols].float()
            val = (_k_loop(xt, w, m, kk) if m in K_MUTATIONS else xt @ w.t()).to(BF)
        dst = gr0 + rows
        keep = dst < M
        dst = dst[keep]
        if epi == "bf16" and mut != "sorted_not_slot":
            dst = out_rows[dst].long()
        out[dst[:, None], cols[None, :]] = val[keep]

    for seq in grouped_schedule(len(tab), tiles_n, cus):
        prev, hole = None, False
        for (tm, tn) in seq:
            ge, gr0, gnr, _ = tab[tm]
            if gnr == 0:
                hole = True
                if mut == "hole_consumed":
                    run(0, 0, 256, tn, 0, 0, None, min(256, M))
                continue
            lost = mut == "skip_after_hole" and hole
            we = prev[0] if (mut == "wrong_expert" and prev is not None) else ge
            xr0 = prev[1] if (mut == "stale_rows" and prev is not None) else gr0
            m = mut if (tm, tn) == last and (mut in K_MUTATIONS or mut == "gate_up_swap") else None
            if not lost:
                run(ge, gr0, gnr, tn, we, xr0, m, 256 if (mut == "wrap_stored" and gnr < 256) else gnr)
            prev, hole = tab[tm], False
    return out


# ---- the tile order of the mirror, observable: one run whose answer depends on it --------------------
def order_probe(cus: int):
    """A table of 2 cus + 8 entries at N = 256 (one n-tile: an entry is a tile) in which the tiles that
    grouped_schedule gives ONE workgroup all name the same chunk of 3 rows (rows 4 b .. 4 b + 2 for
    workgroup b; row 4 b + 3 belongs to no chunk), each with another expert: the i-th tile of a workgroup
    uses expert i.  The chunks of one workgroup overlap on purpose, outside ka_gemm_big_grouped's contract
    for its callers: the same lanes of the same workgroup store the same addresses tile after tile, so what
    remains is the answer of the expert of the workgroup's LAST tile -- if the kernel groups and orders its
    units as the mirror says.  Tiles the mirror wrongly put on one workgroup would race or leave another
    expert's answer.  Returns (tab, M, groups, [last expert of workgroup b])."""
    entries = 2 * cus + 8
    sched = grouped_schedule(entries, 1, cus)
    tab = [None] * entries
    for b, seq in enumerate(sched):
        for i, (tm, tn) in enumerate(seq):
            tab[tm] = (i, 4 * b, 3, 0)
    assert all(t is not None for t in tab)
    return tab, 4 * len(sched), max(len(s) for s in sched), [len(s) - 1 for s in sched]
