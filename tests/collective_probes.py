"""Constructed inputs with exactly known answers for the one-shot collectives of csrc/allreduce.hip
(allreduce_oneshot_kernel, allgather_oneshot_kernel, allreduce_rmsnorm_kernel) and the host side of
parallel/custom_allreduce.py: the case list per world size, per-rank input builders that are deterministic
from (case, world, rank, call index), the expected outputs, the comparators, and a torch emulation of the
three kernels that can be broken on purpose (`mut=`).  Shared by tests/test_collective_probes_cpu.py and
tests/test_collective_probes_gpu.py.  Importable without a GPU.

The emulation (`Emu`) keeps what the kernels keep: `world` ranks with two data halves of `cap` elements
each, one shared epoch (`half = epoch & 1`), the work partition (`chunk = ceil8(ceil(n / nblocks))`, `beg`
and `end` per workgroup, 4096 elements per pass of a workgroup; `rpb = ceil(rows / nblocks)` for the fused
kernel), the staging step (with the split-K slab sum in fp32 rounded to bf16) and the reduce or gather
step over the peers' halves in rank order.  All ranks are perfectly synchronised in it, so it says nothing
about the flag handshake itself; what it gives a mutation is the same meaning it would have in the kernel.

Input families and their tolerances, each derived here and none fitted to a kernel's output:

ledger.  Rank p contributes sign(i) 2^p 2^(k(i) + 16 (call mod 4) - 32) at position i, k(i) in [0, 16).
The sum over ranks is (2^world - 1) 2^(...): at most 8 significant bits, so every partial sum is exact in
fp32 in any order and the result is exact in bf16; exponents run from -32 to 39.  Compared with torch.equal.
k(i) spells the low four hex digits of the vector index i // 8 over the lanes of the vector (and again,
multiplied by 5, over the other four lanes), so a shift by any multiple of 8 elements below 2^19 elements
changes k in at least one lane of every vector: a misplaced chunk cannot reproduce the expected value.  A
missing, doubled or foreign rank changes the factor 2^world - 1, the other half (the call before) carries
a scale 2^16 away, and so do the calls two and three before.

bounded random.  randn rounded to bf16, magnitudes clamped to [2^-10, 2): every value is a multiple of
2^-17 and eight of them sum to less than 16, i.e. at most 21 bits: every partial sum is exact in fp32 in any
order.  The reference is the fp64 sum rounded once to bf16, compared with torch.equal; it catches a sum
that is rounded twice, truncated or accumulated in bf16, which the ledger cannot.  Split-K slab cases use
the window [2^-10, 1) and split <= 9: a rank's slab sum is below 9 and a multiple of 2^-17 (21 bits, exact in
fp32), its bf16 rounding is again a multiple of 2^-17 and below 16, and eight of those stay below 128 (24
bits).  The builder asserts all of this in fp64 (forward and reverse fp32 sums equal the fp64 sum).

free random (plain all-reduce only).  Unclamped randn in bf16, so cancellation is exercised.
|got - want64| <= 2^-8 |want64| + world 2^-23 sum_p |x_p|: one bf16 rounding (half an ulp is at most 2^-8
of the value, as in elementwise_probes.py) plus the fp32 summation error, at most (world - 1) 2^-24
sum |x_p|, with a 2x margin.

fused RMSNorm.  The rank contributions are elementwise_probes.int_slices of integer probe rows (+-1
everywhere, +-128 at one probed element per row: row r probes position r mod len of `fused_probe_positions`,
and the widths that use the second 512-vector slot are run once more with one row per position),
and with split-K each rank's contribution is again int_slices of that, as fp32 or bf16 slabs: all integers
below 256, so slab sums and rank sums are exact.  The residual written back equals bf16(sum + res) exactly
(one fp32 add of two bf16 values, one rounding) and is compared with torch.equal; the output is within
2^-8 |want| of elementwise_probes.rms_want in fp64 (that module's derivation: one bf16 rounding of an fp32
value a few fp32 ulp from the truth).  The bounded-random family is run through it as well, so that a rank
sum that is not rounded to bf16 before the residual add is observable in the residual.

all-gather.  16-bit words rank * 4096 + (call mod 4) * 1024 + h(i) with h(i) = 41 (i // 8) + 5 (i % 8) + 1
mod 1024: a swapped rank order, the other half and a chunk displaced by less than 8192 elements each change
every word.  Compared bit for bit as int16.

Groups.  Every process builds two exchange groups.  "main" has cap_elems = 2^16, so that n = 65536 is n == cap
and `rows * hidden > cap` is a refusal at a small shape.  The fused shapes (64, 4096), (65, 4096) and
(129, 2056) and the one-row-per-probe shapes hold more than 2^16 elements, so they, and at world 2 the 524296-element all-reduce whose
threads loop three times, run on "big" (cap_elems = 2^20) with an epoch sequence of its own.  A chunk of
more than one pass is also launched at every world on "main": n = 4104 with one workgroup, for the
all-reduce and for the all-gather.

Co-residency: a workgroup of a one-shot collective waits for the same workgroup of every peer, so all
world * nblocks workgroups of a call must be resident at once.  Every case keeps world * nblocks <= 256
(asserted in `cases`): 64-workgroup launches at world <= 4, at most 32 at world = 8.
"""
from __future__ import annotations

import torch

from tests import elementwise_probes as ep

BF = ep.BF
SENT = ep.SENT
EPS = ep.EPS
CAP = 1 << 16                  # cap_elems of the group every world builds
BIG_CAP = 1 << 20              # a second group: the fused shapes above CAP elements, the multi-pass all-reduce
BIG_N = 64 * 4096 * 2 + 8      # 64 workgroups, chunk 8200: three passes of 4096 elements
GUARD = 16                     # sentinel elements the emulation keeps behind every output
PASS = 512 * 8                 # elements one workgroup handles per pass
AR_MAX_RANKS = 8
AR_MAX_BLOCKS = 64
AR_SK_BATCH = 4
WORLDS = (2, 3, 4, 8)
RESIDENT_WORKGROUPS = 256
INVALID_VALUE = 1              # hipErrorInvalidValue

AR_WRAPPER_NS = (8, 4096, 4104, 12296, 65536)
GATHER_BYTES = ((4, torch.int32), (8, torch.float32), (16, BF), (24, torch.float32), (1120, BF))
FUSED_SHAPES = ((1, 8), (1, 4104), (3, 8192), (64, 4096), (65, 4096), (129, 2056))
FUSED_SPLITS = (3, 4, 5, 8, 9)
FUSED_PROBE_HIDDENS = (4104, 8192)      # run once more with one row per probed position


def fused_probe_positions(hidden: int):
    """The elements a row can probe: both ends of each of the two 512-vector slots of the fused kernel's
    512 threads, the row's ends, and one element per wave and slot."""
    return ep.rms_probe_positions(hidden, 512, 2)


MUTATIONS = ("rank_lost", "rank_twice", "self_only", "stale_half", "chunk_unrounded", "tail_lost",
             "second_pass_skipped", "gather_order", "gather_pad_leak", "sum_unrounded", "res_unrounded",
             "res_ignored", "norm_of_unadded", "slab_drop", "slab_double", "row_block_overlap", "vec_slot_lost",
             "ss_vec_lost")
_COMMON = ("rank_lost", "rank_twice", "self_only", "stale_half")
_PARTITION = ("chunk_unrounded", "tail_lost", "second_pass_skipped")
MUTATIONS_OF = {
    "ar": _COMMON + _PARTITION,
    "ag": _COMMON + _PARTITION + ("gather_order", "gather_pad_leak"),
    "fused": _COMMON + ("sum_unrounded", "res_unrounded", "res_ignored", "norm_of_unadded", "slab_drop",
                        "slab_double", "row_block_overlap", "vec_slot_lost", "ss_vec_lost"),
}


def max_blocks(world: int) -> int:
    return min(AR_MAX_BLOCKS, RESIDENT_WORKGROUPS // world)


def blocks_for(n: int) -> int:
    """OneShotAllReduce.blocks_for (the GPU module checks this against the class)."""
    return max(1, min(AR_MAX_BLOCKS, (n + PASS - 1) // PASS))


def chunk_of(n: int, nblocks: int) -> int:
    return ((n + nblocks - 1) // nblocks + 7) // 8 * 8


# ====================================================================================================
# Input families
# ====================================================================================================
def ledger_k(i: torch.Tensor) -> torch.Tensor:
    v, j = i // 8, i % 8
    digit = (v >> (4 * (j % 4))) & 15
    return torch.where(j < 4, digit + j, digit * 5 + (v >> 16) + j) % 16


def ledger_sign(i: torch.Tensor) -> torch.Tensor:
    return 1 - 2 * (((i // 8) * 7 + (i % 8) * 3) // 2 % 2)


def _ledger(n: int, factor: float, call: int) -> torch.Tensor:
    i = torch.arange(n)
    mag = torch.ldexp(torch.tensor(float(factor)), ledger_k(i) + 16 * (call % 4) - 32)
    return (mag * ledger_sign(i)).to(BF)


def ledger(n: int, rank: int, call: int) -> torch.Tensor:
    """Rank `rank`'s contribution to call `call`: bf16 [n], powers of two."""
    return _ledger(n, 2.0 ** rank, call)


def ledger_sum(n: int, world: int, call: int) -> torch.Tensor:
    return _ledger(n, 2.0 ** world - 1, call)


def bounded_randn(shape, seed: int, hi: float = 2.0) -> torch.Tensor:
    """randn in bf16 with magnitudes clamped to [2^-10, hi): multiples of 2^-17."""
    x = torch.randn(shape, generator=ep._gen(seed)).to(BF).float()
    top = hi * (1 - 2.0 ** -8)                              # the largest bf16 below a power of two hi
    x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp(2.0 ** -10, top)
    assert torch.equal(x.to(BF).float(), x) and torch.equal((x * 2 ** 17).round(), x * 2 ** 17)
    return x.to(BF)


def exact_sum(parts: torch.Tensor, what: str) -> torch.Tensor:
    """fp64 sum over dim 0 of `parts`, after asserting that the fp32 sum in forward and in reverse order is
    that sum exactly."""
    s64 = parts.double().sum(0)
    fwd = torch.zeros_like(parts[0], dtype=torch.float32)
    rev = torch.zeros_like(fwd)
    for p in range(parts.shape[0]):
        fwd = fwd + parts[p].float()
        rev = rev + parts[parts.shape[0] - 1 - p].float()
    assert torch.equal(fwd.double(), s64) and torch.equal(rev.double(), s64), f"{what}: fp32 sum is not exact"
    return s64


def gather_words(nwords: int, rank: int, call: int) -> torch.Tensor:
    i = torch.arange(nwords)
    h = (41 * (i // 8) + 5 * (i % 8) + 1) % 1024
    return (rank * 4096 + (call % 4) * 1024 + h).to(torch.int16)


# ====================================================================================================
# The case list
# ====================================================================================================
def _op(kind, name, **kw):
    d = dict(kind=kind, name=name, inst="main", via="wrapper", family="ledger", framed=False)
    d.update(kw)
    return d


def _fused_op(world, rows, hidden, split, slab_bf16, with_res, family, tag=""):
    nb = min(rows, AR_MAX_BLOCKS, max_blocks(world))
    via = "wrapper" if nb == min(rows, AR_MAX_BLOCKS) else "direct"
    slab = "" if split == 1 else ("bf16" if slab_bf16 else "fp32")
    return _op("fused", f"fused{tag}-{family}-{rows}x{hidden}-split{split}{slab}-{'res' if with_res else 'nores'}",
               rows=rows, hidden=hidden, split=split, slab_bf16=slab_bf16 or split == 1, with_res=with_res,
               family=family, nblocks=nb, via=via, framed=True, inst="big" if rows * hidden > CAP else "main")


def fused_case_specs():
    """(rows, hidden, split, slab_bf16, family).  The three small shapes take every split with both slab
    types.  The three large ones (over 2^18 elements, where building eight ranks' nested slices costs the
    most) take split 1 and a part of the split settings each, chosen so that every (split, slab type) is run
    at rows per workgroup > 1 at least once.  Rows of the (1, 4104) and (3, 8192) shapes reach only the first
    probe positions, so both widths are run again with one row per probed position."""
    out = []
    for rows, hidden in FUSED_SHAPES[:3]:
        out.append((rows, hidden, 1, True, "int"))
        for split in FUSED_SPLITS:
            for sb in (False, True):
                out.append((rows, hidden, split, sb, "int"))
    for hidden in FUSED_PROBE_HIDDENS:
        rows = len(fused_probe_positions(hidden))
        out += [(rows, hidden, 1, True, "int"), (rows, hidden, 5, False, "int")]
    out += [(64, 4096, 1, True, "int"), (64, 4096, 4, False, "int"), (64, 4096, 5, True, "int"),
            (65, 4096, 1, True, "int"), (65, 4096, 3, True, "int"), (65, 4096, 9, False, "int"),
            (65, 4096, 4, False, "int"), (65, 4096, 5, True, "int"), (65, 4096, 8, False, "int"),
            (129, 2056, 1, True, "int"), (129, 2056, 5, False, "int"), (129, 2056, 8, True, "int"),
            (129, 2056, 3, False, "int"), (129, 2056, 4, True, "int"), (129, 2056, 9, True, "int")]
    out += [(1, 8, 1, True, "bounded"), (1, 4104, 1, True, "bounded"), (1, 4104, 9, True, "bounded"),
            (3, 8192, 1, True, "bounded"), (3, 8192, 5, False, "bounded"), (65, 4096, 1, True, "bounded"),
            (129, 2056, 3, False, "bounded")]
    return out


def _sequence_ops(world):
    """Large, small, large block counts over the three kinds, nothing but the stream between the calls."""
    f = lambda r, h: _fused_op(world, r, h, 1, True, True, "ledger", tag="-seq")   # noqa: E731
    return [
        _op("ar", "seq-ar-65536", n=65536, nblocks=16),
        _op("ag", "seq-ag-16B", nbytes=16, dtype=BF, nblocks=1),
        f(16, 4096),
        _op("ar", "seq-ar-8", n=8, nblocks=1),
        _op("ag", "seq-ag-12296", via="direct", n16=12296, nblocks=4, framed=True),
        f(1, 8),
        _op("ar", "seq-ar-12296", n=12296, nblocks=4),
        _op("ar", "seq-ar-8b", n=8, nblocks=1),
        f(3, 8192),
        _op("ag", "seq-ag-4B", nbytes=4, dtype=torch.int32, nblocks=1),
        _op("ar", "seq-ar-65536b", n=65536, nblocks=16),
    ]


GRAPH_REPLAYS = 4


def _graph_ops(world):
    return [_op("ar", "graph-ar-4096", n=4096, nblocks=1),
            _fused_op(world, 2, 4104, 1, True, True, "ledger", tag="-graph"),
            _op("ag", "graph-ag-24B", nbytes=24, dtype=torch.float32, nblocks=1)]


def refusals():
    """(entry point, overrides of a valid call): each must return hipErrorInvalidValue and launch nothing.
    `world` and `rank` given as offsets are relative to the group's world."""
    out = []
    for fn, nkey in (("ar", "n"), ("ag", "n")):
        out += [(fn, {nkey: 12}), (fn, {nkey: CAP + 8}), (fn, {"nblocks": 0}), (fn, {"nblocks": 65}),
                (fn, {"world": 9}), (fn, {"rank": "world"})]
    out += [("fused", {"nblocks": 0}), ("fused", {"nblocks": 65}), ("fused", {"world": 9}), ("fused", {"rank": "world"}),
            ("fused", {"hidden": 12}), ("fused", {"hidden": 8200}), ("fused", {"rows": 9, "hidden": 8192}),
            ("fused", {"rows": 1, "nblocks": 2}), ("fused", {"split": 0}), ("fused", {"split": 1, "in_bf16": 0})]
    return out


REFUSAL_BASE = {"ar": dict(n=64, nblocks=1), "ag": dict(n=64, nblocks=1),
                "fused": dict(rows=2, hidden=64, nblocks=2, split=1, in_bf16=1)}


def host_refuses(fn: str, world: int, rank: int, cap: int, **a) -> bool:
    """The argument checks of ka_allreduce_oneshot / ka_allgather_oneshot / ka_allreduce_rmsnorm."""
    bad = world < 1 or world > AR_MAX_RANKS or rank < 0 or rank >= world or a["nblocks"] < 1 or a["nblocks"] > AR_MAX_BLOCKS
    if fn in ("ar", "ag"):
        return bad or a["n"] % 8 != 0 or a["n"] > cap
    return (bad or a["hidden"] % 8 != 0 or a["hidden"] > 8192 or a["rows"] * a["hidden"] > cap or a["nblocks"] > a["rows"]
            or a["split"] < 1 or (a["split"] == 1 and not a["in_bf16"]))


def refusal_args(fn: str, over: dict, world: int, rank: int):
    a = dict(REFUSAL_BASE[fn], world=world, rank=rank)
    a.update(over)
    if a["rank"] == "world":
        a["rank"] = a["world"]
    return a


def cases(world: int):
    """[dict(name, kind, ops)] in the order every rank walks them.  kind: "single" (each op launched and
    compared), "sequence" (all ops launched back to back, then compared, then `state` checked), "graph" (the
    ops captured once, replayed GRAPH_REPLAYS times: listed once per replay), "refusals".  Every op carries
    its call index `call` (the epoch before the launch) within its group `inst`."""
    nb = max_blocks(world)
    out = []

    def single(ops):
        ops = ops if isinstance(ops, list) else [ops]
        out.append(dict(name=ops[0]["name"], kind="single", ops=ops))

    for n in AR_WRAPPER_NS:
        for fam in ("ledger", "bounded", "free"):
            single(_op("ar", f"ar-{fam}-{n}", n=n, nblocks=blocks_for(n), family=fam))
    for n, b in ((8, 3), (8, nb), (72, 3), (72, nb), (4104, 1)):
        for fam in ("ledger", "bounded"):
            single(_op("ar", f"ar-direct-{fam}-{n}-nb{b}", n=n, nblocks=b, family=fam, via="direct", framed=True))
    for nbytes, dt in GATHER_BYTES:
        single(_op("ag", f"ag-{nbytes}B", nbytes=nbytes, dtype=dt, nblocks=blocks_for((nbytes + 15) // 16 * 8)))
    for n16, b in ((4104, 2), (12296, 4), (4104, 1)):
        single(_op("ag", f"ag-direct-{n16}-nb{b}", via="direct", n16=n16, nblocks=b, framed=True))
    for rows, hidden, split, sb, fam in fused_case_specs():
        single([_fused_op(world, rows, hidden, split, sb, wr, fam) for wr in (True, False)])
    out.append(dict(name="refusals", kind="refusals", ops=[]))
    out.append(dict(name="sequence", kind="sequence", ops=_sequence_ops(world)))
    g = []
    for rep in range(GRAPH_REPLAYS):
        g += [dict(o, name=f"{o['name']}-replay{rep}") for o in _graph_ops(world)]
    out.append(dict(name="graph", kind="graph", ops=g))
    if world == 2:
        for fam in ("ledger", "bounded"):
            single(_op("ar", f"ar-direct-{fam}-{BIG_N}-nb64", n=BIG_N, nblocks=64, family=fam, via="direct",
                       framed=True, inst="big"))
    calls = {"main": 0, "big": 0}
    sid = 0
    for c in out:
        for o in c["ops"]:
            o["call"], o["sid"] = calls[o["inst"]], sid
            calls[o["inst"]] += 1
            sid += 1
            assert world * o["nblocks"] <= RESIDENT_WORKGROUPS, o["name"]
            cap = BIG_CAP if o["inst"] == "big" else CAP
            if o["kind"] == "fused":
                assert o["rows"] * o["hidden"] <= cap and o["nblocks"] <= o["rows"]
            elif o["kind"] == "ar" or o["via"] == "direct":
                assert o.get("n", o.get("n16")) <= cap
    return out


def launches(world: int, inst: str = "main") -> int:
    return sum(1 for c in cases(world) for o in c["ops"] if o["inst"] == inst)


# ====================================================================================================
# Inputs and expected outputs
# ====================================================================================================
def fused_probe_rows(rows: int, hidden: int, seed: int) -> torch.Tensor:
    """fp32 [rows, hidden]: +-1 everywhere, +-128 at probe position r mod len(probes) of row r."""
    probes = fused_probe_positions(hidden)
    x = (torch.randint(0, 2, (rows, hidden), generator=ep._gen(seed)) * 2 - 1).float()
    r = torch.arange(rows)
    x[r, torch.tensor(probes)[r % len(probes)]] *= ep.RMS_BIG_INT
    return x


def _fused_data(op, world: int):
    rows, hidden, split, call = op["rows"], op["hidden"], op["split"], op["call"]
    seed = ep.case_seed(op["sid"], world, call, rows, hidden, split)
    w = ep.rms_weight(hidden)
    if op["family"] == "ledger":
        contrib = torch.stack([ledger(rows * hidden, p, call).view(rows, hidden) for p in range(world)])
        ins = list(contrib)
        res = torch.zeros(rows, hidden, dtype=BF)
    elif op["family"] == "int":
        P, _ = ep.int_slices(fused_probe_rows(rows, hidden, seed), world, seed + 1)
        ins = []
        if split > 1:
            adj = []
            for p in range(world):
                Q, Pp = ep.int_slices(P[p], split, ep.case_seed(seed, p))
                ins.append(Q.to(BF) if op["slab_bf16"] else Q)
                adj.append(Pp)
            P = torch.stack(adj)
        else:
            ins = [P[p].to(BF) for p in range(world)]
        contrib = P.to(BF)
        assert torch.equal(contrib.float(), P)
        res = (torch.randn(rows, hidden, generator=ep._gen(seed + 2)) * 0.5).clamp(-0.9, 0.9).to(BF)
    else:                                                    # bounded random
        ins, contrib = [], []
        for p in range(world):
            if split > 1:
                Q = bounded_randn((split, rows, hidden), ep.case_seed(seed, p), hi=1.0)
                s = exact_sum(Q, op["name"])
                assert float(s.abs().max()) < 9 and split <= 9
                contrib.append(s.to(BF))                     # fp64 -> fp32 is exact here, so one rounding
                ins.append(Q if op["slab_bf16"] else Q.float())
            else:
                ins.append(bounded_randn((rows, hidden), ep.case_seed(seed, p)))
                contrib.append(ins[-1])
        contrib = torch.stack(contrib)
        res = (torch.randn(rows, hidden, generator=ep._gen(seed + 2)) * 0.5).clamp(-0.9, 0.9).to(BF)
    total = exact_sum(contrib, op["name"])
    assert float(total.abs().max()) < 2.0 ** 40
    xsum = total.to(BF)
    if op["family"] != "bounded":
        assert torch.equal(xsum.double(), total)
    res = res if op["with_res"] else None
    want, wres = ep.rms_want(xsum, w, res)
    return dict(ins=ins, contrib=contrib, res=res, w=w, xsum=xsum, want=want, want_res=wres)


def op_data(op, world: int):
    """Every rank's input and the expected output of one launch; the same on every rank."""
    call, kind = op["call"], op["kind"]
    if kind == "fused":
        return _fused_data(op, world)
    if kind == "ag":
        nw = op["n16"] if op["via"] == "direct" else op["nbytes"] // 2
        words = torch.stack([gather_words(nw, p, call) for p in range(world)])
        return dict(ins=list(words), want=words)
    n, fam = op["n"], op["family"]
    if fam == "ledger":
        return dict(ins=[ledger(n, p, call) for p in range(world)], want=ledger_sum(n, world, call))
    seed = ep.case_seed(op["sid"], world, call, n)
    if fam == "bounded":
        ins = [bounded_randn((n,), ep.case_seed(seed, p)) for p in range(world)]
        return dict(ins=ins, want=exact_sum(torch.stack(ins), op["name"]).to(BF))
    ins = [torch.randn(n, generator=ep._gen(ep.case_seed(seed, p))).to(BF) for p in range(world)]
    x = torch.stack(ins).double()
    return dict(ins=ins, want64=x.sum(0), bound_abs=world * 2.0 ** -23 * x.abs().sum(0))


# ====================================================================================================
# Comparators: lists of (op, what, count, first index, got, want), never an exception, because a rank
# must go on launching what its peers launch
# ====================================================================================================
def _record(op, what, bad, got, want):
    if not bool(bad.any()):
        return []
    i = tuple(bad.nonzero()[0].tolist())
    return [(op["name"], what, int(bad.sum()), i, float(got[i]), float(want[i]))]


def diff_exact(op, what, got, want):
    if got.shape != want.shape:
        return [(op["name"], what + " shape", 1, (), float(got.numel()), float(want.numel()))]
    if got.dtype != want.dtype or got.dtype == BF:
        got, want = got.double(), want.double()
    return _record(op, what, got != want, got, want)


def diff_bound(op, what, got, want64, rel, extra=None):
    """(records, largest |got - want| / bound over the elements with a non-zero bound)."""
    got = got.double()
    bound = rel * want64.abs() + (0.0 if extra is None else extra)
    err = (got - want64).abs()
    ratio = float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    return _record(op, what, ~(err <= bound), got, want64), ratio


def compare(op, data, got):
    """got: dict of CPU tensors.  ar: out (+ in_after, frame_ok when framed); ag: out int16 [world, words]
    (+ frame_ok); fused: out, res (or None), frame_ok.  Returns (records, ratio or None)."""
    rec, ratio = [], None
    if op["framed"] and not got.get("frame_ok", True):
        rec.append((op["name"], "frame", 1, (), 0.0, SENT))
    if op["kind"] == "ar":
        if op["family"] == "free":
            r, ratio = diff_bound(op, "out", got["out"], data["want64"], 2.0 ** -8, data["bound_abs"])
            rec += r
        else:
            rec += diff_exact(op, "out", got["out"], data["want"])
        if "in_after" in got:
            rec += diff_exact(op, "input after the call", got["in_after"], data["ins"][got["rank"]])
    elif op["kind"] == "ag":
        rec += diff_exact(op, "out", got["out"], data["want"])
    else:
        if op["with_res"]:
            rec += diff_exact(op, "residual", got["res"], data["want_res"])
        r, ratio = diff_bound(op, "out", got["out"], data["want"], 2.0 ** -8)
        rec += r
    return rec, ratio


# ====================================================================================================
# The emulation
# ====================================================================================================
def stage_slabs(t: torch.Tensor, split: int, mut=None) -> torch.Tensor:
    """What a rank writes into its half: the bf16 input, or the fp32 sum of its slabs in slab order (in
    batches of AR_SK_BATCH, which does not change the order) rounded to bf16."""
    if split <= 1:
        return t
    s = torch.zeros_like(t[0], dtype=torch.float32)
    for z0 in range(0, split, AR_SK_BATCH):
        for z in range(z0, min(split, z0 + AR_SK_BATCH)):
            if mut == "slab_drop" and z == split - 1:
                continue
            s = s + t[z].float()
    if mut == "slab_double":
        s = s + t[split - 1].float()
    return s.to(BF)


def _trunc_bf16(t: torch.Tensor) -> torch.Tensor:
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


class Emu:
    """`world` ranks in lockstep.  `launch` returns one `got` dict per rank, as `compare` takes them."""

    def __init__(self, world: int, cap: int):
        self.world, self.cap = world, cap
        self.data = torch.zeros(world, 2, cap + GUARD, dtype=BF)
        self.ctr = 0

    # -- the work partition of the all-reduce and the all-gather
    def _blocks(self, n, nblocks, mut):
        per = (n + nblocks - 1) // nblocks
        chunk = per if mut == "chunk_unrounded" else (per + 7) // 8 * 8
        lane = torch.arange(8)
        for b in range(nblocks):
            beg = b * chunk
            end = min(n, beg + chunk)
            if mut == "tail_lost" and beg + chunk > n:
                end = beg                                      # the ragged last chunk is never handled
            if beg >= end:
                continue                                       # a trailing workgroup that owns nothing
            starts = torch.arange(beg, end, 8)                 # a thread moves 8 elements from each start
            if mut == "second_pass_skipped":
                starts = starts[starts - beg < PASS]
            yield (starts[:, None] + lane).flatten()

    def _sources(self, r, mut):
        """[(peer, half offset)] in the order rank r adds or gathers them."""
        w = self.world
        order = list(range(w))
        if mut == "rank_lost":
            order = order[:-1]
        elif mut == "rank_twice":
            order[-1] = 0
        elif mut == "self_only":
            order = [r] * w
        return [(p, 1 if mut == "stale_half" and p != r else 0) for p in order]

    def launch(self, op, data, mut=None, commit=True):
        if mut is not None and mut not in MUTATIONS_OF[op["kind"]]:
            mut = None
        epoch = self.ctr + 1
        half = epoch & 1
        if op["kind"] == "fused":
            extent = op["rows"] * op["hidden"]
        else:
            extent = op["n"] if op["kind"] == "ar" else op.get("n16", (op.get("nbytes", 0) + 15) // 16 * 8)
        saved = None if commit else self.data[:, half, :extent + GUARD].clone()
        got = getattr(self, "_" + op["kind"])(op, data, mut, half)
        if commit:
            self.ctr = epoch
        else:
            self.data[:, half, :extent + GUARD] = saved       # a trial run leaves the halves as they were
        return got

    def _ar(self, op, data, mut, half):
        n, w = op["n"], self.world
        pad = torch.zeros(GUARD, dtype=BF)
        ins = [torch.cat([x, pad]) for x in data["ins"]]
        guard = torch.full((GUARD,), SENT, dtype=BF)
        outs = [torch.cat([torch.full((n,), SENT, dtype=BF) if op["framed"] else data["ins"][r].clone(), guard])
                for r in range(w)]
        blocks = list(self._blocks(n, op["nblocks"], mut))
        for idx in blocks:
            for r in range(w):
                self.data[r, half, idx] = ins[r][idx]
        for idx in blocks:
            sums = {}                                          # ranks that read the same sources get the same sum
            for r in range(w):
                src = tuple(self._sources(r, mut))
                if src not in sums:
                    s = torch.zeros(idx.numel())
                    for p, other in src:
                        s = s + self.data[p, half ^ other, idx].float()
                    sums[src] = s.to(BF)
                outs[r][idx] = sums[src]
        got = []
        for r in range(w):
            g = dict(rank=r, out=outs[r][:n], frame_ok=bool((outs[r][n:] == SENT).all()))
            if op["framed"]:
                g["in_after"] = data["ins"][r]
            got.append(g)
        return got

    def _ag(self, op, data, mut, half):
        w = self.world
        if op["via"] == "direct":
            nw, n16 = op["n16"], op["n16"]
        else:                                                  # OneShotAllReduce.all_gather: 16-byte units, zero padded
            nw = op["nbytes"] // 2
            n16 = (op["nbytes"] + 15) // 16 * 8
        ins = [torch.cat([x, torch.zeros(n16 - nw + GUARD, dtype=torch.int16)]).view(BF) for x in data["ins"]]
        outs = [torch.full((w * n16 + GUARD,), SENT, dtype=BF) for _ in range(w)]
        blocks = list(self._blocks(n16, op["nblocks"], mut))
        for idx in blocks:
            for r in range(w):
                self.data[r, half, idx] = ins[r][idx]
        for idx in blocks:
            for r in range(w):
                for slot, (p, other) in enumerate(self._sources(r, mut)):
                    if mut == "gather_order":
                        p = w - 1 - p
                    outs[r][slot * n16 + idx] = self.data[p, half ^ other, idx]
        got = []
        for r in range(w):
            body = outs[r][:w * n16].view(torch.int16)
            if mut == "gather_pad_leak":                       # the padding is not cut out of every row
                out = body[:w * nw].view(w, nw)
            else:
                out = body.view(w, n16)[:, :nw]
            got.append(dict(rank=r, out=out.contiguous(), frame_ok=bool((outs[r][w * n16:] == SENT).all())))
        return got

    def _fused(self, op, data, mut, half):
        rows, hidden, w = op["rows"], op["hidden"], self.world
        nblocks = op["nblocks"]
        rpb = max(1, rows // nblocks) if mut == "row_block_overlap" else (rows + nblocks - 1) // nblocks
        R = min(rows, nblocks * rpb)                           # workgroup b owns rows [b rpb, min(rows, (b + 1) rpb))
        cols = min(hidden, PASS) if mut == "vec_slot_lost" else hidden
        if mut in ("slab_drop", "slab_double"):
            staged = [stage_slabs(t, op["split"], mut) for t in data["ins"]]
        else:
            staged = data.get("staged")
            if staged is None:
                staged = data["staged"] = [stage_slabs(t, op["split"]) for t in data["ins"]]
        for r in range(w):
            self.data[r, half, :R * hidden] = staged[r].reshape(-1)[:R * hidden]
        wf = data["w"].float()
        got, done = [], {}
        for r in range(w):
            src = tuple(self._sources(r, mut))
            if src in done:                                    # ranks that read the same sources get the same result
                got.append(dict(done[src], rank=r))
                continue
            s = torch.zeros(R, hidden)
            for p, other in src:
                s = s + self.data[p, half ^ other, :R * hidden].view(R, hidden).float()
            aw = s if mut == "sum_unrounded" else s.to(BF).float()
            out = torch.full((rows, hidden), SENT, dtype=BF)
            res = None
            if data["res"] is not None:
                res = data["res"].clone()
            if res is not None and mut != "res_ignored":
                t = aw + res[:R].float()
                v = t.to(BF).float()
                res[:R, :cols] = t.to(BF)[:, :cols]
                if mut == "res_unrounded":
                    res[:R, :cols] = _trunc_bf16(t)[:, :cols]
                    v = t
                if mut == "norm_of_unadded":
                    v = aw.to(BF).float()
            else:
                v = aw.to(BF).float()
            sq = v[:, :cols] * v[:, :cols]
            if mut == "ss_vec_lost":                           # the thread of the row's last vector adds nothing
                sq[:, hidden - 8:] = 0
            ss = sq.sum(1, keepdim=True)
            scale = torch.rsqrt(ss / hidden + EPS)
            out[:R, :cols] = (v * scale * wf).to(BF)[:, :cols]
            done[src] = dict(rank=r, out=out, res=res, frame_ok=True)
            got.append(done[src])
        return got
