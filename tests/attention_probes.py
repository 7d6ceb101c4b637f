"""Probe inputs, high-precision references and comparators for the paged attention kernels.

Importable without a GPU: everything here is plain torch and runs on whatever device the caller
asks for.  `tests/test_attention_probes_cpu.py` proves on the CPU that the probes reject each class
of bookkeeping bug (a lost, stale, doubled or misplaced token, a wrong kv head, a causal mask off by
one); `tests/test_attention_probes_gpu.py` runs the same probes through the HIP kernels.

The kernels fix head_dim 128 and KV block size 16, so this module does too.  Layouts:
k_cache [NB, Hkv, 16, 128], v_cache [NB, Hkv, 128, 16] (csrc/attention.hip).

Input families
  count   Q = 0, V of token t for kv head h is the one-hot e[(t + 5 h) mod 128]: every probability
          is exactly 1 and output dim d is (tokens whose code is d) / context, so one token more or
          less moves some output by at least 1 / ceil(context / 128) relative.
  needle  K, V random; all G query heads of a kv group are 4 K[t*], so the output is V[t*] to within
          1e-6 (asserted on the fp64 reference by the builder): probes every K-side index.
  random  randn Q / K / V.
  ramp    random, plus K[t] += u 60 t / ctx along the query's direction: the running maximum rises
          in every chunk, so every pass rescales and the cross-wave merge sees unequal maxima.
In every family the cache slots of a sequence's last block past its context, block 0 (what the
padding entries of a block table name) and a few blocks no table names hold POISON = 1e4 in K and
V: finite on purpose, so a correct kernel (whose masked probabilities are exact zeros) is unaffected
and a leak is loud.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from ai_agent_kubectl_amd import ops
from ai_agent_kubectl_amd.ops import reference as ref

D = 128
BS = 16
POISON = 1e4
BF = torch.bfloat16
SCALE = D ** -0.5
ROPE_THETA = 5e5
MAX_POS = 4096
FAMILIES = ("count", "needle", "random", "ramp")

# The shapes of tests/test_attention_probes_gpu.py; the CPU self-test walks the same lists.
DECODE_CTXS = (33, 129, 257, 700, 2048)        # 129, 257: one token into a 4-wave workgroup's passes 2, 3
NW2_CTXS = (1, 63, 64, 65, 129, 200)           # 2-wave rows (plus one padding and one 700-token row)
FUSED_CTXS = (1, 2, 33, 129, 257, 700)         # including the new token
CASCADE_NS = (1, 2, 7, 40)                     # shared blocks: odd, even, 20 chunks
CASCADE_OWN = (1, 2, 17, 130, 300)             # own tokens, including the new one
PREFILL_SHAPES = (((5,), (600,)), ((130, 1, 17), (130, 257, 700)), ((65,), (65,)), ((33, 31), (64, 63)))


def shape_id(shape) -> str:
    """pytest id of a PREFILL_SHAPES entry."""
    return "q%s_c%s" % ("-".join(map(str, shape[0])), "-".join(map(str, shape[1])))


ALL_DECODE_CTXS = tuple(sorted(set(DECODE_CTXS) | set(NW2_CTXS) | {700} | set(FUSED_CTXS)
                               | {ns * 16 + own for ns in CASCADE_NS for own in CASCADE_OWN}))


# ------------------------------------------------------------------------------------------------
# references


def gather_tokens(k_cache, v_cache, table_row, n: int):
    """Tokens 0 .. n-1 of one sequence through its block table: K, V as float64 [n, Hkv, 128]."""
    t = torch.arange(n, device=k_cache.device)
    blk = table_row.long()[t // BS]
    off = t % BS
    return k_cache[blk, :, off, :].double(), v_cache[blk, :, :, off].double()


def _attend(q, K, V, qpos, scale: float, emulate: bool):
    """q [n, Hq, 128], K / V [L, Hkv, 128] (float64); query row i sees keys j <= qpos[i].
    emulate: P rounded to bf16 before PV, denominator from the unrounded P, output rounded to bf16
    (the kernels' arithmetic: p_store packs bf16, l is summed in fp32)."""
    hq, hkv = q.shape[1], K.shape[1]
    G = hq // hkv
    Kh = K.transpose(0, 1).repeat_interleave(G, dim=0)          # [Hq, L, 128]
    Vh = V.transpose(0, 1).repeat_interleave(G, dim=0)
    s = torch.einsum("nhd,hld->hnl", q, Kh) * scale
    vis = torch.arange(K.shape[0], device=q.device)[None, :] <= qpos[:, None]
    s = s.masked_fill(~vis[None], float("-inf"))
    smax = s.max(dim=-1, keepdim=True).values if s.shape[-1] else s.new_zeros(s.shape[:-1] + (1,))
    smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
    p = torch.exp(s - smax)
    den = p.sum(dim=-1, keepdim=True)
    if emulate:
        p = p.to(BF).double()
    o = torch.einsum("hnl,hld->hnd", p, Vh)
    o = torch.where(den > 0, o / den.clamp_min(1e-300), torch.zeros_like(o)).transpose(0, 1)
    return o.to(BF).double() if emulate else o


def paged_reference(q, k_cache, v_cache, block_tables, q_starts, ctx_lens, scale: float,
                    emulate: bool = False, mutation: Optional[Callable] = None):
    """Varlen paged attention in float64 -> [T, Hq, 128] float64.  Sequence s owns query rows
    q_starts[s] .. q_starts[s + 1] - 1, the last positions of its ctx_lens[s]-token context; rows
    of empty sequences are zero.  mutation(K, V, ctx, qpos) -> (K, V, qpos) rewrites what one
    sequence attends (the CPU self-test's deliberately wrong references); it is handed one token
    past the context where the last block has room for one."""
    T, hq, _ = q.shape
    out = torch.zeros(T, hq, D, dtype=torch.float64, device=q.device)
    qs, cl = q_starts.tolist(), ctx_lens.tolist()
    for s, ctx in enumerate(cl):
        q0, q1 = qs[s], qs[s + 1]
        if q1 == q0 or ctx == 0:
            continue
        qpos = torch.arange(ctx - (q1 - q0), ctx, device=q.device)
        if mutation is None:
            K, V = gather_tokens(k_cache, v_cache, block_tables[s], ctx)
        else:
            K, V = gather_tokens(k_cache, v_cache, block_tables[s], ctx + (1 if ctx % BS else 0))
            K, V, qpos = mutation(K, V, ctx, qpos)
        out[q0:q1] = _attend(q[q0:q1].double(), K, V, qpos, scale, emulate)
    return out


# ------------------------------------------------------------------------------------------------
# comparators


def assert_exact_to_ulp(got, want64, what: str = ""):
    """|got - want| <= 2^-7 |want| + 1e-6.  For count and needle the exact result is a ratio of
    exactly representable sums; the kernel's own error is acc * (1 / den) in fp32 and one bf16
    rounding, at most one bf16 ulp (2^-7 relative)."""
    g, w = got.double().cpu(), want64.double().cpu()
    assert g.shape == w.shape, (g.shape, w.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    excess = (g - w).abs() - (2.0 ** -7 * w.abs() + 1e-6)
    if excess.max().item() > 0:
        idx = [int(i) for i in torch.unravel_index(excess.argmax(), excess.shape)]
        raise AssertionError(f"{what}: (row, head, dim) = {idx}: got {g[tuple(idx)].item():.6g}, "
                             f"want {w[tuple(idx)].item():.6g}; {(excess > 0).sum().item()} of {excess.numel()} "
                             f"outside one bf16 ulp")


def normalised_error(x, want64):
    """Per (row, head): max_d |x - want| / rms_d(want)."""
    w = want64.double().cpu()
    rms = w.pow(2).mean(dim=-1).sqrt()
    return (x.double().cpu() - w).abs().amax(dim=-1) / rms


def assert_attention_close(got, want64, emulated, what: str = "", factor: float = 4.0) -> float:
    """Per (row, head), max_d |got - want| / rms_d(want) must be at most `factor` x the same
    quantity of the bf16-emulating reference on the same inputs (0.007-0.012 at 129-4096 tokens;
    the factor covers the kernels' summation order over chunks and waves and hardware exp2).
    Returns (and prints) the largest kernel / emulated ratio."""
    assert got.shape == want64.shape == emulated.shape, (got.shape, want64.shape, emulated.shape)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    eg, ee = normalised_error(got, want64), normalised_error(emulated, want64)
    ratio = torch.where(ee > 0, eg / ee, torch.where(eg > 0, torch.full_like(eg, float("inf")), torch.zeros_like(eg)))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"attention_close {what}: kernel/emulated ratio max {worst:.3f}, "
          f"kernel err max {eg.max().item():.4f}, emulated err max {ee.max().item():.4f}")
    if worst > factor:
        r, h = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
        raise AssertionError(f"{what}: (row, head) = ({r}, {h}): normalised error {eg[r, h].item():.4f} is "
                             f"{worst:.2f} x the bf16-emulated reference's {ee[r, h].item():.4f} (limit {factor} x)")
    return worst


def rejects(check: Callable, *args) -> bool:
    """True when the comparator raises on these arguments."""
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------
# probe cases


@dataclass
class Case:
    family: str
    hq: int
    hkv: int
    k_cache: torch.Tensor
    v_cache: torch.Tensor
    block_tables: torch.Tensor          # [S, W] int32; padding entries name block 0 (poison)
    ctx_lens: torch.Tensor              # [S] int32
    q_starts: torch.Tensor              # [S + 1] int32
    q: Optional[torch.Tensor] = None    # [T, Hq, 128] bf16 (unfused ops)
    scale: float = SCALE
    targets: Optional[List[Optional[int]]] = None   # needle: per query row, the token it must return
    # fused kernels: raw (unrotated) projection output; the caches lack the new token
    qkv: Optional[torch.Tensor] = None          # [S, (hq + 2 hkv) 128] bf16 (of partials: their ordered sum)
    partials: Optional[torch.Tensor] = None     # [split, S, width] fp32 | bf16
    positions: Optional[torch.Tensor] = None
    slots: Optional[torch.Tensor] = None
    cos_sin: Optional[torch.Tensor] = None
    shared: int = 0                             # leading table entries every row shares (cascade)
    qlens: List[int] = field(default_factory=list)

    def to(self, device) -> "Case":
        kw = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        return Case(**kw)

    @property
    def rows(self) -> torch.Tensor:
        """Query rows of non-empty sequences (padding rows are compared separately: zeros)."""
        cl, qs = self.ctx_lens.tolist(), self.q_starts.tolist()
        return torch.tensor([r for s, c in enumerate(cl) if c > 0 for r in range(qs[s], qs[s + 1])], dtype=torch.long)

    def qkv_input(self):
        return self.qkv if self.partials is None else ops.SplitK(self.partials, self.partials.shape[0])

    def reference(self, q=None, k_cache=None, v_cache=None, emulate=False, mutation=None):
        return paged_reference(self.q if q is None else q, self.k_cache if k_cache is None else k_cache,
                               self.v_cache if v_cache is None else v_cache, self.block_tables, self.q_starts,
                               self.ctx_lens, self.scale, emulate, mutation)

    def rope_append(self, rope_kv_write=ops.rope_kv_write):
        """Fused cases: (rotated q, k_cache, v_cache) after the unfused RoPE + KV append on clones."""
        k2, v2 = self.k_cache.clone(), self.v_cache.clone()
        q = rope_kv_write(self.qkv, self.positions, self.cos_sin, self.slots, k2, v2, self.hq, self.hkv, D)
        return q, k2, v2


def needle_targets(ctx: int) -> List[int]:
    """Chunk (32), half-chunk (16) and pass (32 NW, NW = 2 and 4) boundaries, the middle (where the
    block mutations of the self-test strike) and the two newest tokens."""
    cand = {0, 15, 16, 31, 32, 63, 64, 127, 128, ctx // 2, ctx - 2, ctx - 1}
    return sorted(t for t in cand if 0 <= t < ctx)


def needle_rows(ctxs: Sequence[int]) -> List[Tuple[int, Optional[int]]]:
    """One row per (context, target)."""
    return [(c, t) for c in ctxs for t in (needle_targets(c) if c > 0 else [None])]


def _onehot_codes(hkv: int, t0: int, n: int) -> torch.Tensor:
    """V of tokens t0 .. t0 + n - 1: [Hkv, n, 128] bf16 one-hot at (t + 5 h) mod 128."""
    code = (torch.arange(t0, t0 + n)[None, :] + 5 * torch.arange(hkv)[:, None]) % D
    return torch.nn.functional.one_hot(code, D).to(BF)


def _randn(gen, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=gen).to(BF)


def _unit(x: torch.Tensor) -> torch.Tensor:
    x = x.float()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-6)


def _kv(family: str, hkv: int, ctx: int, gen, t0: int = 0):
    K = _randn(gen, hkv, ctx, D)
    V = _onehot_codes(hkv, t0, ctx) if family == "count" else _randn(gen, hkv, ctx, D)
    return K, V


def _ramp(K: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """K [Hkv, ctx, 128] += u [Hkv, 128] * 60 t / ctx."""
    ctx = K.shape[1]
    t = torch.arange(ctx, dtype=torch.float32)[None, :, None]
    return (K.float() + u[:, None, :] * 60.0 * t / ctx).to(BF)


def _page(Ks, Vs, ctxs, hkv, width, gen, shared: int = 0, spare: int = 3, skip_last: bool = False):
    """Scatter per-row dense K / V [Hkv, ctx, 128] into poisoned paged caches through randomly
    permuted block tables.  Block 0 and `spare` more blocks stay in no table.  shared: the first
    `shared` table entries are the same physical blocks in every non-empty row (their contents
    taken from the first such row).  skip_last: the newest token's slot stays poisoned (the fused
    kernels append it themselves)."""
    need = [(c + BS - 1) // BS for c in ctxs]
    W = max(max(need), 1) + (0 if width == "tight" else 5)
    nb = 1 + spare + shared + sum(max(n - shared, 0) for n in need)
    perm = (1 + torch.randperm(nb - 1, generator=gen)).tolist()
    shared_ids, k = perm[:shared], shared
    bt = torch.zeros(len(ctxs), W, dtype=torch.int32)
    kc = torch.full((nb, hkv, BS, D), POISON, dtype=BF)
    vc = torch.full((nb, hkv, D, BS), POISON, dtype=BF)
    for s, c in enumerate(ctxs):
        if c == 0:
            continue
        assert need[s] > shared or shared == 0
        ids = shared_ids + perm[k:k + need[s] - shared]
        k += need[s] - shared
        bt[s, :need[s]] = torch.tensor(ids, dtype=torch.int32)
        n = c - 1 if skip_last else c
        t = torch.arange(n)
        blk, off = bt[s].long()[t // BS], t % BS
        kc[blk, :, off, :] = Ks[s][:, :n].transpose(0, 1)
        vc[blk, :, :, off] = Vs[s][:, :n].transpose(0, 1)
    return kc, vc, bt


def _assert_needles(case: Case, want64: torch.Tensor, k_cache=None, v_cache=None):
    """Builder's own check: on the fp64 reference every needle row returns V[t*] to 1e-6."""
    kc = case.k_cache if k_cache is None else k_cache
    vc = case.v_cache if v_cache is None else v_cache
    qs, cl = case.q_starts.tolist(), case.ctx_lens.tolist()
    G = case.hq // case.hkv
    for s, c in enumerate(cl):
        for r in range(qs[s], qs[s + 1]):
            t = case.targets[r]
            if c == 0 or t is None:
                continue
            _, V = gather_tokens(kc, vc, case.block_tables[s], c)
            err = (want64[r] - V[t].repeat_interleave(G, dim=0)).abs().max().item()
            assert err <= 1e-6, f"needle row {r} (ctx {c}, target {t}): fp64 reference is {err:.3g} from V[t*]"


def decode_case(family: str, hq: int, hkv: int, rows: Sequence, width: str = "wide", seed: int = 0,
                device="cpu") -> Case:
    """`ops.attention_decode` inputs.  rows: contexts (0 = padding row), or for needle
    (context, target) pairs as `needle_rows` makes them."""
    assert family in FAMILIES and hq % hkv == 0
    gen = torch.Generator().manual_seed(seed)
    G = hq // hkv
    rows = [r if isinstance(r, tuple) else (r, None) for r in rows]
    ctxs = [c for c, _ in rows]
    Ks, Vs, qs, targets = [], [], [], []
    for c, t in rows:
        K, V = _kv(family, hkv, c, gen)
        q = _randn(gen, hq, D)
        if family == "count":
            q = torch.zeros(hq, D, dtype=BF)
        elif family == "needle" and c > 0:
            t = c - 1 if t is None else t
            q = (4 * K[:, t]).repeat_interleave(G, dim=0)
        elif family == "ramp" and c > 0:
            K = _ramp(K, _unit(q[::G]))
        Ks.append(K), Vs.append(V), qs.append(q), targets.append(t)
    kc, vc, bt = _page(Ks, Vs, ctxs, hkv, width, gen)
    case = Case(family, hq, hkv, kc, vc, bt, torch.tensor(ctxs, dtype=torch.int32),
                torch.arange(len(rows) + 1, dtype=torch.int32), q=torch.stack(qs),
                targets=targets if family == "needle" else None, qlens=[1] * len(rows))
    if family == "needle":
        _assert_needles(case, case.reference())
    return case.to(device)


def _rope_inverse(y: torch.Tensor, cs_row: torch.Tensor) -> torch.Tensor:
    """x with rope(x) = y at the position whose cos | sin row is cs_row (float64)."""
    half = D // 2
    c, s = cs_row[:half].double(), cs_row[half:].double()
    y1, y2 = y[..., :half].double(), y[..., half:].double()
    return torch.cat([y1 * c + y2 * s, y2 * c - y1 * s], dim=-1)


def _split_partials(target_bf: torch.Tensor, split: int, bf16: bool, gen):
    """[split, S, width] partials whose sum in the kernels' order (k = 0, 1, ... in fp32, rounded to
    bf16) is returned with them.  Slices 1.. are multiples of 1/8 in [-4, 4] and slice 0 the rest, so
    for targets that are small multiples of 1/8 (the count family's zeros and one-hots) every slice
    and the sum are exact in either format, and a lost or doubled slice shows."""
    S, width = target_bf.shape
    noise = torch.randint(-32, 33, (split - 1, S, width), generator=gen).float() / 8
    P = torch.cat([(target_bf.float() - noise.sum(0))[None], noise]).to(BF if bf16 else torch.float32)
    acc = P[0].float().clone()
    for k in range(1, split):
        acc += P[k].float()
    return P, acc.to(BF)


def fused_case(family: str, hq: int, hkv: int, rows: Sequence, width: str = "wide", seed: int = 0,
               split: int = 0, shared: int = 0, device="cpu") -> Case:
    """`ops.decode_attention_rope` inputs: the caches hold the ctx - 1 earlier (rotated) tokens, the
    new token's raw q / k / v are in qkv (or in `|split|` split-K partials, bf16 when split < 0); a
    row of context 0 is a padding row (slot -1).  shared > 0: cascade, every row's first `shared`
    blocks are the same physical blocks."""
    assert family in ("count", "needle", "random") and hq % hkv == 0
    gen = torch.Generator().manual_seed(seed)
    G = hq // hkv
    rows = [r if isinstance(r, tuple) else (r, None) for r in rows]
    ctxs = [c for c, _ in rows]
    cs = ref.rope_cos_sin(MAX_POS, D, ROPE_THETA)
    Ksh, Vsh = _kv(family, hkv, shared * BS, gen)
    Ks, Vs, raw, targets = [], [], [], []
    for c, t in rows:
        assert c == 0 or c > shared * BS
        own = max(c - shared * BS, 0)
        K, V = _kv(family, hkv, own, gen, t0=shared * BS)
        if c > 0:
            K, V = torch.cat([Ksh, K], dim=1), torch.cat([Vsh, V], dim=1)
        rq, rk, rv = _randn(gen, hq, D), _randn(gen, hkv, D), _randn(gen, hkv, D)
        if family == "count":
            rq = torch.zeros(hq, D, dtype=BF)
            rv = V[:, c - 1] if c > 0 else torch.zeros(hkv, D, dtype=BF)
        elif family == "needle" and c > 0:
            t = c - 1 if t is None else t
            if t == c - 1:      # the new token: q = 4 k before and so after the rotation
                rq = (4 * rk).repeat_interleave(G, dim=0)
            else:
                rq = _rope_inverse(4 * K[:, t].float(), cs[c - 1]).to(BF).repeat_interleave(G, dim=0)
        Ks.append(K), Vs.append(V), targets.append(t)
        raw.append(torch.cat([rq.reshape(-1), rk.reshape(-1), rv.reshape(-1)]))
    kc, vc, bt = _page(Ks, Vs, ctxs, hkv, width, gen, shared=shared, skip_last=True)
    qkv = torch.stack(raw)
    P = None
    if split:
        P, qkv2 = _split_partials(qkv, abs(split), split < 0, gen)
        if family == "count":   # the zero q part and the one-hot v part survive the reduction exactly
            assert torch.equal(qkv2[:, :hq * D], qkv[:, :hq * D])
            assert torch.equal(qkv2[:, (hq + hkv) * D:], qkv[:, (hq + hkv) * D:])
        qkv = qkv2
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    slots = torch.tensor([int(bt[s, (c - 1) // BS]) * BS + (c - 1) % BS if c > 0 else -1 for s, c in enumerate(ctxs)],
                         dtype=torch.int32)
    case = Case(family, hq, hkv, kc, vc, bt, ctx, torch.arange(len(rows) + 1, dtype=torch.int32),
                targets=targets if family == "needle" else None, qkv=qkv, partials=P,
                positions=(ctx - 1).clamp(min=0), slots=slots, cos_sin=cs, shared=shared, qlens=[1] * len(rows))
    if family == "needle":
        q, k2, v2 = case.rope_append(ref.rope_kv_write)
        _assert_needles(case, case.reference(q, k2, v2), k2, v2)
    return case.to(device)


def cascade_rows(family: str, ns: int, S: int, owns: Sequence[int] = CASCADE_OWN):
    """S - 1 rows of ns shared blocks + an own part cycling through `owns`, then a padding row.
    Needle targets alternate between the shared prefix and the own part."""
    rows = []
    for i in range(S - 1):
        c = ns * BS + owns[i % len(owns)]
        cand = [t for t in (0, ns * BS - 1, ns * BS, c - 1, c - 2, 15, 16, 31, 32, ns * 8) if 0 <= t < c]
        rows.append((c, cand[(i + i // len(owns)) % len(cand)] if family == "needle" else None))
    return rows + [(0, None)]


def prefill_case(family: str, hq: int, hkv: int, qlens: Sequence[int], ctxs: Sequence[int], width: str = "wide",
                 seed: int = 0, device="cpu") -> Case:
    """`ops.attention_prefill` inputs: sequence s has qlens[s] query rows at the last positions of
    its ctxs[s]-token context.  Needle: query row at position p targets p and p - 1 in turn; one row
    per sequence (where p + 1 is in the context) carries the needles of p AND p + 1, equally strong:
    it must return V[p], and a mask that lets p + 1 through returns about half of each."""
    assert family in FAMILIES and hq % hkv == 0
    gen = torch.Generator().manual_seed(seed)
    G = hq // hkv
    Ks, Vs, qs, targets = [], [], [], []
    for n, c in zip(qlens, ctxs):
        assert 0 < n <= c
        K, V = _kv(family, hkv, c, gen)
        q = _randn(gen, n, hq, D)
        if family == "count":
            q = torch.zeros(n, hq, D, dtype=BF)
        elif family == "needle":
            for i in range(n):
                p = c - n + i
                t = p - 1 if (i % 2 and p > 0) else p
                needle = 4 * K[:, t].float()
                if i == n // 2 and p + 1 < c:
                    t, needle = p, 4 * (K[:, p].float() + K[:, p + 1].float())
                q[i] = needle.to(BF).repeat_interleave(G, dim=0)
                targets.append(t)
        elif family == "ramp":
            K = _ramp(K, _unit(q[-1, ::G]))
        Ks.append(K), Vs.append(V), qs.append(q)
    kc, vc, bt = _page(Ks, Vs, list(ctxs), hkv, width, gen)
    starts = torch.tensor([0] + torch.tensor(list(qlens)).cumsum(0).tolist(), dtype=torch.int32)
    case = Case(family, hq, hkv, kc, vc, bt, torch.tensor(list(ctxs), dtype=torch.int32), starts, q=torch.cat(qs),
                targets=targets if family == "needle" else None, qlens=list(qlens))
    if family == "needle":
        _assert_needles(case, case.reference())
    return case.to(device)


def running_count(hq: int, hkv: int, qlens: Sequence[int], ctxs: Sequence[int]) -> torch.Tensor:
    """The count family's exact answer, from the codes alone (no attention): [T, Hq, 128] float64."""
    G = hq // hkv
    out = []
    for n, c in zip(qlens, ctxs):
        if c == 0:
            out.append(torch.zeros(n, hq, D, dtype=torch.float64))
            continue
        cum = _onehot_codes(hkv, 0, c).double().cumsum(dim=1)                # [Hkv, ctx, 128]
        pos = torch.arange(c - n, c)
        out.append((cum[:, pos] / (pos + 1)[None, :, None]).transpose(0, 1).repeat_interleave(G, dim=1))
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------
# reference mutations (CPU self-test): what a kernel with a bookkeeping bug would compute


class Mutation(NamedTuple):
    name: str
    fn: Callable                                    # (K, V, ctx, qpos) -> (K, V, qpos)
    defined: Callable[[int, int], bool]             # (ctx, hkv) -> bool


def _all(K, V):
    return K, V, torch.full((1,), K.shape[0] - 1, device=K.device)


def _mid_block(ctx: int, span: int) -> int:
    """First of `span` adjacent full blocks at (or nearest below) the middle of the context."""
    return min((ctx // 2) // BS, ctx // BS - span)


def _drop_last(K, V, ctx, qpos):
    return _all(K[:ctx - 1], V[:ctx - 1])


def _stale_token(K, V, ctx, qpos):
    return _all(K[:ctx + 1], V[:ctx + 1])


def _zero_v(K, V, ctx, qpos):
    V = V[:ctx].clone()
    V[ctx // 2] = 0
    return _all(K[:ctx], V)


def _double_token(K, V, ctx, qpos):
    t = ctx // 2
    return _all(torch.cat([K[:ctx], K[t:t + 1]]), torch.cat([V[:ctx], V[t:t + 1]]))


def _drop_block(K, V, ctx, qpos):
    b = _mid_block(ctx, 1) * BS
    keep = torch.cat([torch.arange(b), torch.arange(b + BS, ctx)]).to(K.device)
    return _all(K[keep], V[keep])


def _swap_v_blocks(K, V, ctx, qpos):
    b = _mid_block(ctx, 2) * BS
    V = V[:ctx].clone()
    V[b:b + 2 * BS] = torch.cat([V[b + BS:b + 2 * BS], V[b:b + BS]])
    return _all(K[:ctx], V)


def _next_kv_head(K, V, ctx, qpos):
    return _all(K[:ctx].roll(-1, dims=1), V[:ctx].roll(-1, dims=1))


DECODE_MUTATIONS = [
    Mutation("last_token_dropped", _drop_last, lambda ctx, hkv: ctx >= 2),
    Mutation("stale_token_attended", _stale_token, lambda ctx, hkv: ctx % BS != 0),
    Mutation("v_of_one_token_zeroed", _zero_v, lambda ctx, hkv: True),
    # (a one-token context attends that token with weight 1 however often it is counted)
    Mutation("token_counted_twice", _double_token, lambda ctx, hkv: ctx >= 2),
    Mutation("mid_block_dropped", _drop_block, lambda ctx, hkv: ctx > 32),
    Mutation("v_blocks_swapped", _swap_v_blocks, lambda ctx, hkv: ctx > 32),
    Mutation("next_kv_head_read", _next_kv_head, lambda ctx, hkv: hkv > 1),
]

# Prefill: the causal mask off by one.  (+1 lets the stale slot past the context through where the
# last block has room for it.)
PREFILL_MUTATIONS = [
    Mutation("causal_mask_minus_one", lambda K, V, ctx, qpos: (K[:ctx], V[:ctx], qpos - 1), lambda ctx, hkv: True),
    Mutation("causal_mask_plus_one", lambda K, V, ctx, qpos: (K, V, qpos + 1), lambda ctx, hkv: True),
]
