"""Probe inputs, an fp64 reference, a partition mirror and a breakable emulation of the persistent
decode kernel (csrc/decode_persistent.hip) at geometries of a few MB.

Importable without a GPU (plain torch).  `tests/test_decode_probes_cpu.py` proves on the CPU that
the probes reject each class of bookkeeping bug; `tests/test_decode_probes_gpu.py` runs the same
case list through `ops.decode_persistent`.

Ledger inputs (compared with torch.equal)
  h0 is +-1 and the norm gains are in {+-1, 2, 4}, so x = bf16(+-1 rstd g) = +-g whatever the last
  bits of rstd (mean square exactly 1).  Every weight row is designed against the activation it will
  meet: a few random small integers in every 512-column chunk, then one or two correction entries
  that bring the row's sum to its target for BOTH sequences of a B = 2 launch (sequence 1 is
  sequence 0 with some signs flipped, so a column where the two agree and one where they differ
  solve for any pair of targets of equal parity).  Every chunk of a row contributes a non-zero
  amount different from the row's other chunks, so a dropped, doubled, stale or shifted 1-KB piece
  changes the sum.  Targets:
    q / k rows  the inverse rotation (cos / sin table of {0, +-1}, a different pattern per position,
                row 0 the identity) of the needle codes 64 (e_a + e_b);
    v rows      m_d sigma_d: magnitudes per (layer, kv head, dim), signs per token;
    O / down    'flip': 0 or -2 res_i, so the residual stays +-1 and the next norm is exact again;
                'free' (last layer only): any integer |.| <= 100, read back from ws.res and h_out;
                'zero': the phase is switched off;
    gate        {0, 32, 64}: g / (1 + exp(-g)) is exactly g in fp32, so act = g u; up: +-1 .. +-4.
  Down weights are integers / 32 (act is a multiple of 32).

Attention families (the leader's attention; q, k_new and v_new are ledger integers)
  needle  cached K are codes 64 (e_a + e_b), a distinct pair per token, kv head and layer; the
          winner leads by >= 4096 before scaling (>= 362 after), every other probability is an exact
          0 in fp32 and attn = V[t*] bit for bit, carried through O into the residual.
  count   Wq = 0, V = 2 e[(t + 5 h + l) mod 128]: attn is one bf16 rounding of count / context.
  random, ramp, rope   soft softmax (L = 1, later phases off), ws.attn against the bf16-emulating
          reference with attention_probes.assert_attention_close; rope uses the model's table
          (theta 5e5) and also compares the appended K to one bf16 ulp.
Caches: POISON = 1e4 in block 0, in blocks no table names and past each context; block tables are
random permutations; K / V differ per layer and kv head.

The emulation (`step(..., mode="emu")`) computes the same step organised as the kernel is: rows by
wave through `Part` (the mirror of the kernel's work partition), 512-column pieces, chunk c of the
context on wave c mod 8, the first chunk of a wave from the ring.  `mut` breaks it on purpose.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from ai_agent_kubectl_amd.ops import reference as ref
from tests import attention_probes as ap

BF = torch.bfloat16
F64 = torch.float64
NW, HD, KBS = 8, 128, 16
POISON = ap.POISON
EPS = 1e-5
SCALE = HD ** -0.5
SYNC_BYTES, ERR_BYTE, MAXB = 4096, 4032, 2
CUS = 256                       # MI355X; the launcher never uses more than 256 workgroups
STREAMS = ("qkv", "o", "gu", "down")


def rb(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (through fp32, as the kernel's f2bf), back as float64."""
    return x.float().to(BF).double()


# ------------------------------------------------------------------------------------------------
# the launcher's host checks and the kernel's work partition, mirrored


@dataclass(frozen=True)
class Geo:
    H: int
    hq: int
    hkv: int
    I: int

    @property
    def gq(self):
        return self.hq // self.hkv

    @property
    def qkvn(self):
        return (self.hq + 2 * self.hkv) * HD


def pd_ring(gq: int, B: int) -> int:
    return (16 if B == 1 else 14) if gq > 4 else 16


def ring_down(B: int, rg: int) -> int:
    return rg if B == 1 else min(rg, 12)


def _kb(n: int) -> int:
    return (n + 1023) // 1024 * 1024


def scratch_bytes(gr: int) -> int:
    return 10240 + gr * 256 + 1024 + 2 * 8 * gr * 4 + 64 + (0 if gr > 4 else 8 * gr * 128 * 4)


def lds_bytes(B: int, H: int, hq: int, I: int, gq: int) -> int:
    xh, xs = _kb(max(H, hq * 128) * 2), _kb(max(H, I, hq * 128) * 2)
    scr = _kb(scratch_bytes(8)) if gq > 4 else 29 * 1024
    rg = pd_ring(gq, B)
    ring = max(B * (xs if B == 1 else xh), scr)
    ring_d = ring if B == 1 else B * xs
    red = max(ring + NW * rg * 1024, ring_d + NW * ring_down(B, rg) * 1024)
    return red + 64 + B * 1024


def max_b(H: int, hq: int, I: int, gq: int) -> int:
    if H <= 8192 and lds_bytes(2, H, hq, I, gq) <= 160 * 1024:
        return 2
    return 1 if lds_bytes(1, H, hq, I, gq) <= 160 * 1024 else 0


def launcher_grid(hkv: int, cap: Optional[int] = None, cus: int = CUS) -> int:
    if cap is not None:
        cus = min(cus, max(1, cap))
    return (min(cus, 256) // hkv) * hkv


def refuses(geo: Geo, B: int, cap: Optional[int] = None, cus: int = CUS) -> bool:
    """True when ka_decode_persistent returns an error without launching."""
    H, hq, hkv, I = geo.H, geo.hq, geo.hkv, geo.I
    if B < 1 or B > MAXB or hkv <= 0 or hq % hkv or hq // hkv > 8 or hkv > 16 or H % 512 or I % 512 or (hq * 128) % 512:
        return True
    if H > 16384 or B > max_b(H, hq, I, hq // hkv):
        return True
    G = launcher_grid(hkv, cap, cus)
    if G < hkv or G // hkv < B + 1:
        return True
    p = Part(geo, B, G)
    return p.qkv_per_wave > 64 or p.h_per_wave > 64 or 2 * p.i_per_wave > 64 or p.o_per_wave > 64


def ws_bytes(geo: Geo) -> int:
    return SYNC_BYTES + MAXB * (geo.H * 4 + geo.qkvn * 2 + geo.hq * HD * 2 + geo.I * 2) + 1024


def ws_views(ws: torch.Tensor, geo: Geo) -> Dict[str, torch.Tensor]:
    """Views of a uint8 workspace: sync 4096 B | res fp32 [2][H] | qkv bf16 [2][(hq + 2 hkv) 128]
    (before RoPE) | attn bf16 [2][hq 128] | act bf16 [2][I]; the error word at byte 4032."""
    assert ws.dtype == torch.uint8 and ws.numel() >= ws_bytes(geo)
    o = SYNC_BYTES
    out = {"err": ws[ERR_BYTE:ERR_BYTE + 4].view(torch.int32)}
    for name, dt, n in (("res", torch.float32, geo.H), ("qkv", BF, geo.qkvn), ("attn", BF, geo.hq * HD), ("act", BF, geo.I)):
        nb = MAXB * n * (4 if dt == torch.float32 else 2)
        out[name] = ws[o:o + nb].view(dt).view(MAXB, n)
        o += nb
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


class Part:
    """The kernel's work partition for a geometry, batch and grid."""

    def __init__(self, geo: Geo, B: int, G: int):
        self.geo, self.B, self.G = geo, B, G
        self.pg = G // geo.hkv
        self.nwaves = G * NW
        self.qkv_rows = (geo.gq + 2) * HD
        self.qkv_per_wave = _cdiv(self.qkv_rows, self.pg * NW)
        self.h_per_wave = _cdiv(geo.H, self.nwaves)
        self.i_per_wave = _cdiv(geo.I, self.nwaves)
        self.o_per_wave = _cdiv(geo.H, (G - B * geo.hkv) * NW) if G > B * geo.hkv else 1 << 30
        self.RG = pd_ring(geo.gq, B)
        self.RGD = ring_down(B, self.RG)
        self.PJ = 2 if self.RG >= 16 else 1      # blocks of a wave's first chunk prefetched into its ring

    def ring(self, stream: str) -> int:
        return self.RGD if stream == "down" else self.RG

    def hb(self, stream: str) -> int:
        return self.ring(stream) // 2

    def kc(self, stream: str) -> int:
        g = self.geo
        return {"qkv": g.H, "o": g.hq * HD, "gu": g.H, "down": g.I}[stream] // 512

    def per_wave(self, stream: str) -> int:
        return {"qkv": self.qkv_per_wave, "o": self.o_per_wave, "gu": 2 * self.i_per_wave, "down": self.h_per_wave}[stream]

    def qkv_grow(self, grp: int, r: int) -> int:
        g = self.geo
        if r < g.gq * HD:
            return grp * g.gq * HD + r
        if r < (g.gq + 1) * HD:
            return g.hq * HD + grp * HD + (r - g.gq * HD)
        return (g.hq + g.hkv) * HD + grp * HD + (r - (g.gq + 1) * HD)

    def rows(self, stream: str, wg: int, wave: int) -> List[int]:
        """Global weight rows of one wave, in the order lane 0, 1, ..."""
        g, gw = self.geo, wg * NW + wave
        grp, ig = wg // self.pg, wg % self.pg
        if stream == "qkv":
            q0 = (ig * NW + wave) * self.qkv_per_wave
            return [self.qkv_grow(grp, r) for r in range(q0, min(self.qkv_rows, q0 + self.qkv_per_wave))]
        if stream == "o":
            if ig < self.B:
                return []
            o0 = ((grp * (self.pg - self.B) + ig - self.B) * NW + wave) * self.o_per_wave
            return list(range(o0, min(g.H, o0 + self.o_per_wave)))
        if stream == "gu":
            g0 = gw * self.i_per_wave
            ng = max(0, min(g.I, g0 + self.i_per_wave) - g0)
            return [(g.I + g0 + i // 2) if i & 1 else g0 + i // 2 for i in range(2 * ng)]
        o0 = gw * self.h_per_wave
        return list(range(o0, min(g.H, o0 + self.h_per_wave)))

    def store_rows(self, stream: str, wg: int) -> List[int]:
        """The qkv rows / act elements a workgroup stores as 4-byte pairs, in store order."""
        if stream == "qkv":
            w0 = (wg % self.pg) * NW * self.qkv_per_wave
            return [self.qkv_grow(wg // self.pg, i) for i in range(w0, min(self.qkv_rows, w0 + NW * self.qkv_per_wave))]
        w0 = wg * NW * self.i_per_wave
        return list(range(w0, min(self.geo.I, w0 + NW * self.i_per_wave)))

    @functools.lru_cache(maxsize=None)
    def counts(self, stream: str) -> Tuple[int, ...]:
        return tuple(len(self.rows(stream, wg, w)) for wg in range(self.G) for w in range(NW))

    @functools.lru_cache(maxsize=None)
    def all_rows(self, stream: str) -> torch.Tensor:
        """Every row some wave owns (each exactly once, asserted)."""
        rows = [r for wg in range(self.G) for w in range(NW) for r in self.rows(stream, wg, w)]
        assert len(rows) == len(set(rows)), f"{stream}: a row has two owners"
        return torch.tensor(rows, dtype=torch.long)

    def target_wave(self, stream: str, partial: bool = False) -> Optional[Tuple[int, int]]:
        """The wave the stream mutations strike: the last one with the most rows, or (partial) the
        last one with fewer rows than the others but at least one."""
        cnt = self.counts(stream)
        full = max(cnt)
        if full == 0:
            return None
        want = [i for i, c in enumerate(cnt) if (0 < c < full if partial else c == full)]
        return (want[-1] // NW, want[-1] % NW) if want else None

    @staticmethod
    def chunk_in_ring(c: int) -> bool:
        """A wave's first chunk (c < 8) comes from the ring-prefetched blocks, later ones from global."""
        return c < NW


@functools.lru_cache(maxsize=None)
def part(geo: Geo, B: int, G: int) -> Part:
    return Part(geo, B, G)


# ------------------------------------------------------------------------------------------------
# cases


@dataclass(frozen=True)
class Case:
    name: str
    geo: Geo
    B: int
    L: int
    family: str                      # needle | count | random | ramp | rope
    ncached: Tuple[int, ...]         # per sequence; -1: a padding row (pos 0, slot -1, ctx 0)
    targets: Tuple = ()              # needle: per sequence a cached token index or "new"
    o: str = "flip"                  # zero | flip | free
    mlp: str = "flip"                # zero (w13 = w2 = 0) | flip | free (down free in the last layer)
    cap: Optional[int] = None        # KA_PD_GRID
    seed: int = 0

    @property
    def G(self):
        return launcher_grid(self.geo.hkv, self.cap)

    @property
    def part(self) -> Part:
        return part(self.geo, self.B, self.G)

    @property
    def exact(self) -> bool:
        return self.family == "needle"


GA = Geo(1024, 4, 2, 1536)     # chunk counts 2 / 1 / 2 / 3
GB8 = Geo(512, 8, 1, 512)      # GQA 8; ring 14 at B = 2
GC = Geo(1536, 12, 3, 1024)    # G = 255
GD = Geo(1536, 12, 2, 1024)    # six q rows in GR 8
GE = Geo(512, 4, 4, 2048)      # GQA 1
GF = Geo(1024, 4, 2, 1024)     # G = 4: 64 rows per wave
GG = Geo(512, 28, 4, 512)      # GQA 7: seven pieces per O row, one batch of the 14-slot ring at B = 2
NCACHED = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 273, 600)


def leader_targets(n: int) -> List:
    """First / last token of a chunk, the last ring token and the first global one, the last cached
    token, the new token."""
    cand = [0, 31, 32, 255, 256, 287, n - 1]
    out = sorted({t for t in cand if 0 <= t < n})
    return out + ["new"]


def _cases() -> List[Case]:
    cs: List[Case] = []
    k = 0

    def add(name, geo, B, L, family, nc, tg=(), **kw):
        nonlocal k
        k += 1
        cs.append(Case(name, geo, B, L, family, tuple(nc), tuple(tg), seed=1000 + k, **kw))

    # streams and layers: every geometry, B = 1 / 2 (unequal lengths, or row 1 padding), L = 1 / 3
    for gi, geo in enumerate((GA, GB8, GC, GD, GE)):
        n0, n1 = (17, 40, 33, 273, 5)[gi], (70, 3, 257, 16, 0)[gi]
        add(f"g{gi}_b1_l3_down", geo, 1, 3, "needle", (n0,), (n0 // 2,), o="flip", mlp="free")
        add(f"g{gi}_b1_l1_o", geo, 1, 1, "needle", (n1,), ("new",), o="free", mlp="zero")
        add(f"g{gi}_b2_l3_down", geo, 2, 3, "needle", (n0, n1), (n0 - 1, "new"), o="flip", mlp="free")
        add(f"g{gi}_b2_l3_o", geo, 2, 3, "needle", (n1, n0), ("new", 0), o="free", mlp="zero")
        add(f"g{gi}_b2_pad_l1", geo, 2, 1, "needle", (n0, -1), (0, "new"), o="flip", mlp="free")
    add("gqa7_b2_l2_down", GG, 2, 2, "needle", (33, 17), (32, "new"), o="flip", mlp="free")
    add("gqa7_b2_l1_o", GG, 2, 1, "needle", (16, 257), (15, 256), o="free", mlp="zero")
    # small grids through KA_PD_GRID (chosen for the coverage assertions of the CPU module)
    for geo, B, cap in SMALL_GRIDS:
        add(f"grid{cap}_H{geo.H}_hq{geo.hq}_hkv{geo.hkv}_I{geo.I}_b{B}", geo, B, 2, "needle",
            (33, 17)[:B], (32, "new")[:B], o="flip", mlp="free", cap=cap)
        add(f"grid{cap}_H{geo.H}_hq{geo.hq}_hkv{geo.hkv}_I{geo.I}_b{B}_o", geo, B, 1, "needle",
            (16, 31)[:B], (15, 0)[:B], o="free", mlp="zero", cap=cap)
    # the attention leader: every context length x every target (B = 1, GQA 2)
    for n in NCACHED:
        for t in leader_targets(n):
            add(f"needle_n{n}_t{t}", GA, 1, 1, "needle", (n,), (t,), o="free", mlp="zero")
    # ... B = 2 with unequal lengths on GQA 8 (ring 14: one prefetched block), GQA 6 and GQA 1
    for geo, tag in ((GB8, "gqa8"), (GD, "gqa6"), (GE, "gqa1")):
        for (n0, n1), (t0, t1) in (((257, 16), (256, 15)), ((32, 273), ("new", 255)), ((600, 0), (287, "new")),
                                   ((17, -1), (16, "new"))):
            add(f"needle_{tag}_n{n0}_{n1}", geo, 2, 1, "needle", (n0, n1), (t0, t1), o="free", mlp="zero")
    add("needle_gqa8_b1_n600", GB8, 1, 1, "needle", (600,), (256,), o="free", mlp="zero")
    add("needle_l3_n257", GA, 2, 3, "needle", (257, 33), (255, 32), o="flip", mlp="flip")
    # soft families (later phases off)
    for n in (0, 17, 256, 600):
        add(f"count_n{n}", GA, 1, 3 if n == 17 else 1, "count", (n,), o="zero", mlp="zero")
    add("count_gqa8_b2", GB8, 2, 1, "count", (273, 31), o="zero", mlp="zero")
    add("count_gqa6_pad", GD, 2, 1, "count", (257, -1), o="zero", mlp="zero")
    for fam in ("random", "ramp"):
        add(f"{fam}_n273", GA, 1, 1, fam, (273,), o="zero", mlp="zero")
        add(f"{fam}_n600_b2", GA, 2, 1, fam, (600, 33), o="zero", mlp="zero")
        add(f"{fam}_gqa8_b2", GB8, 2, 1, fam, (257, 600), o="zero", mlp="zero")
        add(f"{fam}_gqa6", GD, 1, 1, fam, (600,), o="zero", mlp="zero")
    add("rope_n273_b2", GA, 2, 1, "rope", (273, 17), o="zero", mlp="zero")
    add("rope_gqa8", GB8, 1, 1, "rope", (600,), o="zero", mlp="zero")
    return cs


# (geometry, B, KA_PD_GRID): GF at 4 workgroups has 64 O rows and 64 gate / up rows per wave
SMALL_GRIDS = ((GF, 1, 4), (GA, 1, 6), (GA, 2, 24), (GB8, 2, 3), (GB8, 2, 11), (GB8, 1, 3), (GE, 1, 8), (GE, 2, 36),
               (GC, 2, 9), (GD, 2, 37), (Geo(512, 4, 1, 512), 1, 2), (Geo(512, 4, 2, 512), 2, 23),
               (Geo(1024, 8, 1, 512), 1, 15), (Geo(1024, 8, 1, 512), 2, 15), (Geo(512, 12, 3, 2048), 1, 27),
               (Geo(512, 8, 1, 2048), 2, 8), (Geo(512, 12, 2, 512), 1, 4), (GB8, 2, 23))
CASES = _cases()
# launches back to back on one workspace, B alternating 1, 2, 1 (stale sync words, residual or ob)
BACK_TO_BACK = ("g0_b1_l3_down", "g0_b2_l3_down", "g0_b1_l1_o")


def case_by_name(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


# ------------------------------------------------------------------------------------------------
# inputs


@dataclass
class Inputs:
    case: Case
    h0: torch.Tensor                 # [B, H] bf16
    layers: List[Dict[str, torch.Tensor]]   # wqkv, wo, w13, w2, ln1, ln2 (bf16)
    k_cache: torch.Tensor            # [L, NB, hkv, 16, 128] bf16
    v_cache: torch.Tensor            # [L, NB, hkv, 128, 16] bf16
    pos: torch.Tensor
    slot: torch.Tensor
    ctx: torch.Tensor
    bt: torch.Tensor                 # [B, W] int32
    cos_sin: torch.Tensor            # [P, 128] fp32
    info: Dict = field(default_factory=dict)

    def to(self, device) -> "Inputs":
        mv = lambda v: v.to(device) if isinstance(v, torch.Tensor) else v
        return Inputs(self.case, mv(self.h0), [{k: mv(v) for k, v in l.items()} for l in self.layers], mv(self.k_cache),
                      mv(self.v_cache), mv(self.pos), mv(self.slot), mv(self.ctx), mv(self.bt), mv(self.cos_sin), self.info)


def ledger_table(P: int, gen) -> torch.Tensor:
    """cos | sin rows of {0, +-1}: a quarter turn count per pair and position; row 0 the identity."""
    k = torch.randint(0, 4, (P, HD // 2), generator=gen)
    k[0] = 0
    assert torch.unique(k, dim=0).shape[0] == P, "two positions share a rotation pattern"
    c = torch.tensor([1.0, 0.0, -1.0, 0.0])[k]
    s = torch.tensor([0.0, 1.0, 0.0, -1.0])[k]
    return torch.cat([c, s], dim=-1).float()


_PAIRS = torch.combinations(torch.arange(HD), 2)      # 8128 pairs


def _code(pair_perm: torch.Tensor, t: int) -> torch.Tensor:
    a, b = _PAIRS[pair_perm[t]]
    v = torch.zeros(HD, dtype=F64)
    v[a] = v[b] = 64.0
    return v


def design(A: torch.Tensor, T: torch.Tensor, gen, what: str, noise: int = 3) -> torch.Tensor:
    """Integer weight rows W [N, K] with W A[b] = T[:, b] for every sequence b: `noise` random entries
    of +-1 .. +-3 in every 512-column chunk, then a correction on a column where the sequences agree
    (and, B = 2, one where they differ).  Every chunk of a row contributes a non-zero amount unlike
    the row's other chunks (K > 512); |W| <= 256 (bf16 integers)."""
    B, K = A.shape
    N, KC = T.shape[0], K // 512
    a0 = A[0]
    if B == 2:
        assert torch.equal(a0.abs(), A[1].abs()), f"{what}: the sequences' activations differ in magnitude"
        assert ((T[:, 0] - T[:, 1]) % 2 == 0).all(), f"{what}: targets of unequal parity"
        same = ((a0.abs() == 1) & (a0 == A[1])).nonzero().flatten()
        anti = ((a0.abs() == 1) & (a0 == -A[1])).nonzero().flatten()
    else:
        same, anti = (a0.abs() == 1).nonzero().flatten(), torch.empty(0, dtype=torch.long)
    assert len(same), f"{what}: no unit column to correct on"
    W = torch.zeros(N, K, dtype=F64)
    todo = torch.arange(N)
    for _ in range(60):
        n = len(todo)
        Wt = torch.zeros(n, K, dtype=F64)
        for c in range(KC):
            pos = c * 512 + torch.randint(0, 512, (n, noise), generator=gen)
            val = torch.randint(1, 4, (n, noise), generator=gen) * (2 * torch.randint(0, 2, (n, noise), generator=gen) - 1)
            Wt.scatter_add_(1, pos, val.double())
        d = T[todo] - Wt @ A.T
        ar = torch.arange(n)
        p = same[torch.randint(0, len(same), (n,), generator=gen)]
        if B == 1 or not len(anti):
            assert B == 1 or torch.equal(d[:, 0], d[:, 1]), f"{what}: the sequences agree everywhere but their targets differ"
            Wt[ar, p] += d[:, 0] * a0[p]
        else:
            q = anti[torch.randint(0, len(anti), (n,), generator=gen)]
            Wt[ar, p] += (d[:, 0] + d[:, 1]) / 2 * a0[p]
            Wt[ar, q] += (d[:, 0] - d[:, 1]) / 2 * a0[q]
        C = torch.einsum("nkj,bkj->bnk", Wt.view(n, KC, 512), A.view(B, KC, 512))
        assert torch.equal(C.sum(-1).T, T[todo]), what
        good = (Wt.abs().amax(dim=1) <= 256) & (Wt == Wt.round()).all(dim=1)
        if KC > 1:
            good &= (C != 0).all(dim=2).all(dim=0)
            for c1 in range(KC):
                for c2 in range(c1 + 1, KC):
                    good &= (C[:, :, c1] != C[:, :, c2]).all(dim=0)
        W[todo[good]] = Wt[good]
        todo = todo[~good]
        if not len(todo):
            return W
    raise AssertionError(f"{what}: {len(todo)} rows found no design")


def _signs(gen, *shape):
    return (2 * torch.randint(0, 2, shape, generator=gen) - 1).double()


def _par(T0: torch.Tensor, gen, spread: int) -> torch.Tensor:
    """Targets for two sequences of equal parity: [N, 2]."""
    return torch.stack([T0, T0 + 2 * torch.randint(-spread, spread + 1, T0.shape, generator=gen).double()], dim=1)


def build(case: Case) -> Inputs:
    """The inputs of one launch (CPU tensors).  Deterministic in case.seed."""
    gen = torch.Generator().manual_seed(case.seed)
    geo, B, L, fam = case.geo, case.B, case.L, case.family
    H, hq, hkv, I, gq = geo.H, geo.hq, geo.hkv, geo.I, geo.gq
    pad = [n < 0 for n in case.ncached]
    nc = [max(n, 0) for n in case.ncached]
    pos = [0 if pad[b] else nc[b] for b in range(B)]
    # h0: +-1; sequence 1 agrees with sequence 0 on every fourth column and elsewhere half the time
    s0 = _signs(gen, H)
    flip = (torch.rand(H, generator=gen) < 0.5) & (torch.arange(H) % 4 != 0)
    h0 = torch.stack([s0, torch.where(flip, -s0, s0)])[:B]
    # block tables and poisoned caches
    need = [0 if pad[b] else nc[b] // KBS + 1 for b in range(B)]
    NB = 1 + 3 + sum(need)
    perm = (1 + torch.randperm(NB - 1, generator=gen)).tolist()
    bt = torch.zeros(B, max(need) + 2, dtype=torch.int32)
    k0 = 0
    for b in range(B):
        bt[b, :need[b]] = torch.tensor(perm[k0:k0 + need[b]], dtype=torch.int32)
        k0 += need[b]
    slot = [-1 if pad[b] else int(bt[b, nc[b] // KBS]) * KBS + nc[b] % KBS for b in range(B)]
    kc = torch.full((L, NB, hkv, KBS, HD), POISON, dtype=BF)
    vc = torch.full((L, NB, hkv, HD, KBS), POISON, dtype=BF)
    cos_sin = ref.rope_cos_sin(max(pos) + 2, HD, ap.ROPE_THETA) if fam == "rope" else ledger_table(max(pos) + 2, gen)
    gains = torch.tensor([1.0, -1.0, 2.0, 4.0], dtype=F64)
    layers, info = [], {"attn_int": fam == "needle"}
    res = h0.clone()
    for l in range(L):
        last = l == L - 1
        g1 = gains[torch.randint(0, 4, (H,), generator=gen)]
        g2 = gains[torch.randint(0, 4, (H,), generator=gen)]
        g1[::4][torch.rand(H // 4, generator=gen) < 0.5] = 1.0      # unit columns the sequences agree on
        g2[::4][torch.rand(H // 4, generator=gen) < 0.5] = 1.0
        g1[1::4][torch.rand(H // 4, generator=gen) < 0.5] = -1.0
        g2[1::4][torch.rand(H // 4, generator=gen) < 0.5] = -1.0
        x = res * g1
        # ---- cached tokens and the new token's q / k / v ----
        Tq = torch.zeros(B, hq, HD, dtype=F64)
        Tk = torch.zeros(B, hkv, HD, dtype=F64)
        Tv = torch.zeros(B, hkv, HD, dtype=F64)
        attn = torch.zeros(B, hq, HD, dtype=F64)
        vmag = torch.randint(1, 4, (hkv, HD), generator=gen).double()
        vmag[:, torch.randperm(HD, generator=gen)[:48]] = 1.0
        for b in range(B):
            n = nc[b]
            t = torch.arange(n)
            blk, off = bt[b].long()[t // KBS], t % KBS
            for h in range(hkv):
                if fam == "needle":
                    pp = torch.randperm(len(_PAIRS), generator=gen)
                    K = torch.stack([_code(pp, i) for i in range(n + 1)])
                    V = vmag[h] * _signs(gen, n + 1, HD)
                    assert torch.unique(V, dim=0).shape[0] == n + 1
                    tg = case.targets[b]
                    tg = n if tg == "new" else tg
                    assert 0 <= tg <= n
                    qstar, attn[b, h * gq:(h + 1) * gq] = K[tg], V[tg]
                else:
                    K = torch.randn(n + 1, HD, generator=gen).to(BF).double()
                    V = torch.randn(n + 1, HD, generator=gen).to(BF).double()
                    knew, vnew, qstar = (torch.randint(-2, 3, (HD,), generator=gen).double() for _ in range(3))
                    if b == 1:      # the parity of sequence 0's targets (see design)
                        match = lambda new, old: new + ((new - old) % 2)
                        knew, vnew, qstar = match(knew, Tk[0, h]), match(vnew, Tv[0, h]), match(qstar, Tq[0, h * gq])
                    K[n], V[n] = knew, vnew
                    if fam == "count":
                        V = 2.0 * torch.nn.functional.one_hot((torch.arange(n + 1) + 5 * h + l) % HD, HD).double()
                    if fam == "ramp" and n:     # along the rotated q: the running maximum rises in every chunk
                        u = _rope(qstar, cos_sin[pos[b]])
                        u = u / u.norm().clamp_min(1e-6)
                        K[:n] = (K[:n] + u[None] * 60.0 * torch.arange(n)[:, None] / n).to(BF).double()
                kc[l, blk, h, off] = K[:n].to(BF)
                vc[l, blk, h, :, off] = V[:n].to(BF)
                if fam == "needle":
                    Tq[b, h * gq:(h + 1) * gq] = ap._rope_inverse(qstar, cos_sin[pos[b]])
                    Tk[b, h] = ap._rope_inverse(K[n], cos_sin[pos[b]])
                elif fam == "count":
                    Tk[b, h] = K[n]
                else:           # raw integers; what they rotate to is the reference's business
                    Tq[b, h * gq:(h + 1) * gq] = qstar
                    Tk[b, h] = K[n]
                Tv[b, h] = V[n]
        T = torch.cat([Tq.reshape(B, -1), Tk.reshape(B, -1), Tv.reshape(B, -1)], dim=1).T.contiguous()   # [QKVN, B]
        if B == 2 and fam == "needle":
            assert ((T[:, 0] - T[:, 1]) % 2 == 0).all()
        wqkv = design(x, T, gen, f"{case.name} wqkv[{l}]")
        if fam == "count":
            wqkv[:hq * HD] = 0
        # ---- O ----
        mode_o = case.o if (last or case.o != "free") else "flip"
        if mode_o == "zero":
            wo, upd = torch.zeros(H, hq * HD, dtype=F64), torch.zeros(B, H, dtype=F64)
        else:
            assert fam == "needle"
            if mode_o == "flip":
                f = (torch.rand(H, generator=gen) < 0.25).double()
                upd = -2.0 * res * f
            else:
                t0 = torch.randint(-100, 101, (H,), generator=gen).double()
                same_attn = B == 2 and torch.equal(attn[0], attn[1])
                upd = (_par(t0, gen, 0 if same_attn else 20).T[:B] if B == 2 else t0[None]).contiguous()
            wo = design(attn.reshape(B, -1), upd.T.contiguous(), gen, f"{case.name} wo[{l}]")
        res = res + upd
        # ---- gate / up, down ----
        mode_d = "zero" if case.mlp == "zero" or (mode_o == "free") else ("free" if (case.mlp == "free" and last) else "flip")
        if mode_d == "zero":
            w13, w2 = torch.zeros(2 * I, H, dtype=F64), torch.zeros(H, I, dtype=F64)
        else:
            x2 = res * g2
            gate = 32.0 * torch.randint(0, 3, (I,), generator=gen).double()
            mu = torch.randint(1, 5, (I,), generator=gen).double()
            up = torch.stack([mu * _signs(gen, I) for _ in range(B)], dim=1)
            w13 = design(x2, torch.cat([gate[:, None].expand(I, B), up]).contiguous(), gen, f"{case.name} w13[{l}]")
            act32 = (gate[None] / 32.0) * up.T                         # act / 32
            if mode_d == "flip":
                upd = -2.0 * res * (torch.rand(H, generator=gen) < 0.25).double()
            else:
                t0 = torch.randint(-100, 101, (H,), generator=gen).double()
                upd = (_par(t0, gen, 20).T if B == 2 else t0[None]).contiguous()
            w2 = design(act32.contiguous(), upd.T.contiguous(), gen, f"{case.name} w2[{l}]") / 32.0
            res = res + upd
        mats = dict(wqkv=wqkv, wo=wo, w13=w13, w2=w2, ln1=g1, ln2=g2)
        for k_, v_ in mats.items():
            assert torch.equal(v_.to(BF).double(), v_), f"{case.name} {k_}[{l}] is not bf16"
        layers.append({k_: v_.to(BF) for k_, v_ in mats.items()})
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    ctx = [0 if pad[b] else nc[b] + 1 for b in range(B)]
    return Inputs(case, h0.to(BF), layers, kc, vc, i32(pos), i32(slot), i32(ctx), bt, cos_sin, info)


# ------------------------------------------------------------------------------------------------
# the step: fp64 reference (mode "ref") and the partition-organised emulation (mode "emu")


@dataclass
class Mut:
    name: str
    stream: Optional[str] = None


def _norm(res, g, eps=EPS):
    rstd = torch.rsqrt(res.pow(2).mean(dim=-1, keepdim=True) + eps)
    return rb(res * rstd * g[None])


def _rope(x, cs_row):
    half = HD // 2
    c, s = cs_row[:half].double(), cs_row[half:].double()
    x1, x2 = x[..., :half], x[..., half:]
    return rb(torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1))


def _stream(p: Optional[Part], name: str, W: torch.Tensor, X: torch.Tensor, mut: Optional[Mut], applied: List[str]):
    """Row results [B, N] (fp64, unrounded) of W [N, K] against the activation rows X [B, K].  With a
    partition: piece by piece (row, 512-column chunk), every wave's rows; a row no wave owns stays NaN."""
    W = W.double()
    if p is None:
        return X @ W.T
    Bn, K = X.shape
    N, KC = W.shape[0], K // 512
    R = torch.full((Bn, N), float("nan"), dtype=F64)
    hit = mut is not None and mut.stream == name
    if not hit:
        own = p.all_rows(name)
        R[:, own] = (X @ W.T)[:, own]
        return R
    Wc, Xc = W.view(N, KC, 512), X.view(Bn, KC, 512)
    C = torch.einsum("nkj,bkj->bnk", Wc, Xc)
    if mut.name == "leaders_get_o_rows":   # the O rows dealt to every workgroup; a leader never runs its share
        opw_all = _cdiv(N, p.G * NW)
        owner = torch.arange(N) // opw_all // NW
        lost = (owner % p.pg) < p.B
        applied.append(mut.name)
        return torch.where(lost[None], torch.zeros_like(R), C.sum(-1))
    own = p.all_rows(name)
    R[:, own] = C.sum(-1)[:, own]
    m = mut.name
    tw = p.target_wave(name, partial=(m == "lose_last_row_partial"))
    if tw is None:
        return R
    rows = p.rows(name, *tw)
    n, RG = len(rows), p.ring(name)
    r, c = rows[n // 2], KC - 1
    if m == "drop_chunk":
        R[:, r] -= C[:, r, c]
    elif m == "double_chunk":
        R[:, r] += C[:, r, c]
    elif m == "stale_chunk":          # the ring slot still holds the piece RG pieces earlier
        j = n * KC - 1
        if j < RG:
            return R
        r, c, rs, cs_ = rows[j // KC], j % KC, rows[(j - RG) // KC], (j - RG) % KC
        R[:, r] += torch.einsum("j,bj->b", Wc[rs, cs_], Xc[:, c]) - C[:, r, c]
    elif m == "rotate_x":
        if KC == 1:
            return R
        R[:, rows] = torch.einsum("nkj,bkj->bn", Wc[rows], Xc.roll(-1, dims=1))
    elif m == "row_shift":
        if n < 2:
            return R
        R[:, rows[:-1]] = R[:, rows[1:]].clone()
    elif m in ("lose_last_row", "lose_last_row_partial"):
        R[:, rows[-1]] = 0.0
    elif m == "lose_row63":
        if n < 64:
            return R
        R[:, rows[63]] = 0.0
    elif m == "swap_x_rows":
        if Bn < 2:
            return R
        R[:, rows] = R[:, rows].flip(0)
    elif m == "swap_gate_up":
        g = [x_ for x_ in rows if x_ < N // 2]
        u = [x_ + N // 2 for x_ in g]
        R[:, g], R[:, u] = R[:, u].clone(), R[:, g].clone()
    elif m == "pair_shift":           # strikes the stores, not the rows: see _pair_shift
        return R
    else:
        raise KeyError(m)
    applied.append(m)
    return R


def _pair_shift(p: Part, name: str, v: torch.Tensor, applied: List) -> torch.Tensor:
    """The struck workgroup's 4-byte stores of result pairs (qkv, act [B, n]) land one pair late: its
    last pair is lost, its first keeps what was there (0)."""
    rr = p.store_rows(name, p.target_wave(name)[0])
    if len(rr) < 4:
        return v
    old = v[:, rr].clone()
    v[:, rr[2:]] = old[:, :-2]
    v[:, rr[:2]] = 0.0
    applied.append("pair_shift")
    return v


def _attend_ref(q, kn, vn, kc_l, vc_l, bt_row, n, h, emulate):
    """q [Gq, 128], the n cached tokens of kv head h through the table plus the new token."""
    t = torch.arange(n)
    blk, off = bt_row.long()[t // KBS], t % KBS
    K = torch.cat([kc_l[blk, h, off].double(), kn[None]])
    V = torch.cat([vc_l[blk, h, :, off].double().reshape(n, HD), vn[None]])
    return ap._attend(q[None], K[:, None], V[:, None], torch.tensor([n]), SCALE, emulate)[0]


def _lead(q, kn, kc_l, bt_row, n, h) -> float:
    """Smallest lead (log2 units) of the winning score over every other visible token, the new one
    included, among the q rows of one kv head."""
    t = torch.arange(n)
    blk, off = bt_row.long()[t // KBS], t % KBS
    s = (q @ torch.cat([kc_l[blk, h, off].double(), kn[None]]).T) * (SCALE * 1.4426950408889634)
    if s.shape[1] < 2:
        return math.inf
    top = s.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def _attend_emu(p: Part, q, kn, vn, kc_l, vc_l, kc_prev, vc_prev, bt_row, n, h, m: Optional[str], applied):
    """The leader's attention: chunk c of 32 tokens on wave c mod 8, blocks bt[2 c] and (if it holds
    a cached token) bt[2 c + 1], online softmax per wave with P rounded to bf16 for P V, the waves
    and the new token merged in fp32."""
    sl2 = SCALE * 1.4426950408889634
    Gq = q.shape[0]
    nch = (n + 31) // 32
    mask_n = n
    if m == "lose_last_cached" and n % 32 == 1:    # the chunk count taken from n - 1: the last token, alone in
        nch, _ = nch - 1, applied.append(m)        # its chunk, is never visited (the mask is right)
    if m == "mask_early" and n >= 1:
        mask_n, _ = n - 1, applied.append(m)
    if m == "mask_late" and n % 32 != 0:
        mask_n, _ = n + 1, applied.append(m)
    parts = []
    for w in range(NW):
        mw = torch.full((Gq,), -math.inf, dtype=F64)
        lw = torch.zeros(Gq, dtype=F64)
        ow = torch.zeros(Gq, HD, dtype=F64)
        for c in range(w, nch, NW):
            if m == "lose_chunk8" and c == 8:
                applied.append(m)
                continue
            t0 = 32 * c
            b0 = int(bt_row[2 * c])
            b1 = int(bt_row[2 * c + 1]) if t0 + 16 < n else b0
            vis = torch.arange(32) + t0 < mask_n
            if m == "poison_leak" and c == nch - 1 and t0 + 16 >= n:   # the table's next entry read, unmasked
                b1, vis, _ = int(bt_row[2 * c + 1]), torch.ones(32, dtype=torch.bool), applied.append(m)
            Ks, Vs = [], []
            for j, bb in enumerate((b0, b1)):
                src_k, src_v = kc_l, vc_l
                if m == "ring_prev_layer" and p.chunk_in_ring(c) and j < p.PJ and kc_prev is not None:
                    src_k, src_v, _ = kc_prev, vc_prev, applied.append(m)
                Ks.append(src_k[bb, h].double())
                Vs.append(src_v[bb, h].double().T)
            K, V = torch.cat(Ks), torch.cat(Vs)
            if m == "lose_second_block" and t0 + 16 < n and c == (n - 17) // 32:
                vis = vis & (torch.arange(32) < 16)
                applied.append(m)
            s = (q @ K.T) * sl2
            s = s.masked_fill(~vis[None], -math.inf)
            mn = torch.maximum(mw, s.amax(dim=1))
            alpha = torch.where(torch.isinf(mn), torch.zeros_like(mn), torch.exp2(mw - mn))
            pr = torch.where(torch.isinf(s), torch.zeros_like(s), torch.exp2(s - mn[:, None])).float().double()
            pr = torch.where(pr < 2.0 ** -149, torch.zeros_like(pr), pr)       # fp32 underflow
            lw = lw * alpha + pr.sum(dim=1)
            ow = ow * alpha[:, None] + rb(pr) @ V
            mw = mn
        parts.append((mw, lw, ow))
    sn = (q @ kn) * sl2
    M = sn.clone()
    for mw, _, _ in parts:
        M = torch.maximum(M, mw)
    wnew = {"no_new_token": 0.0, "double_new_token": 2.0}.get(m, 1.0)
    if wnew != 1.0:
        applied.append(m)
    den = wnew * torch.exp2(sn - M)
    num = den[:, None] * vn[None]
    for mw, lw, ow in parts:
        e = torch.where(torch.isinf(mw), torch.zeros_like(mw), torch.exp2(mw - M)).float().double()
        den = den + e * lw
        num = num + e[:, None] * ow
    return rb(num / den.clamp_min(1e-300)[:, None])


LAYER_MUTS = ("prev_layer_weights", "prev_layer_gains", "residual_not_carried", "hout_before_last_down")


def step(inp: Inputs, mode: str = "ref", mut: Optional[Mut] = None, emulate: bool = False):
    """One persistent step.  Returns (out, applied): out has qkv / attn / act / res of the last layer
    [B, .] (float64), h_out [B, H], the caches after the append (bf16) and (mode "ref", needle) the
    smallest lead of a winning score over all layers, sequences and heads; `applied` lists the
    mutations that found something to break.  mode "ref": plain fp64 (emulate: the attention's P and
    output rounded as the kernels round them); mode "emu": organised by the kernel's partition."""
    case = inp.case
    geo, B, L = case.geo, case.B, case.L
    H, hq, hkv, I, gq = geo.H, geo.hq, geo.hkv, geo.I, geo.gq
    p = case.part if mode == "emu" else None
    m = mut.name if mut is not None else None
    assert mut is None or mode == "emu"
    applied: List = []
    kc, vc = inp.k_cache.clone(), inp.v_cache.clone()
    res = inp.h0.double()
    out = {"needle_gap": math.inf}
    for l in range(L):
        lw, lg = inp.layers[l], inp.layers[l]
        if l > 0 and m == "prev_layer_weights":
            lw, _ = inp.layers[l - 1], applied.append(m)
        if l > 0 and m == "prev_layer_gains":
            lg, _ = inp.layers[l - 1], applied.append(m)
        if l > 0 and m == "residual_not_carried":
            res, _ = inp.h0.double(), applied.append(m)
        x = _norm(res, lg["ln1"].double())
        qkv = rb(_stream(p, "qkv", lw["wqkv"], x, mut, applied))
        qkv = _pair_shift(p, "qkv", qkv, applied) if m == "pair_shift" and mut.stream == "qkv" else qkv
        attn = torch.zeros(B, hq * HD, dtype=F64)
        for b in range(B):
            sb = b
            pos, slot, ctx, btr = int(inp.pos[b]), int(inp.slot[b]), int(inp.ctx[b]), inp.bt[b]
            if B == 2 and m == "other_seq_table":
                btr, _ = inp.bt[1 - b], applied.append(m)
            if B == 2 and m == "other_seq_pos":
                pos, _ = int(inp.pos[1 - b]), applied.append(m)
            if B == 2 and m == "other_seq_ctx":
                ctx, _ = int(inp.ctx[1 - b]), applied.append(m)
            n = max(ctx - 1, 0)
            cs = inp.cos_sin[pos]
            qh = qkv[sb, :hq * HD].view(hq, HD)
            kh = qkv[sb, hq * HD:(hq + hkv) * HD].view(hkv, HD)
            vh = qkv[sb, (hq + hkv) * HD:].view(hkv, HD)
            qr, kr = _rope(qh, cs), _rope(kh, cs)
            sl = (l + 1) % L if (m == "other_layer_slab" and L > 1) else l
            if sl != l:
                applied.append(m)
            for h in range(hkv):
                hr = (h + 1) % hkv if (m == "next_kv_head" and hkv > 1) else h
                if hr != h:
                    applied.append(m)
                qg = qr[h * gq:(h + 1) * gq]
                if p is None:
                    o = _attend_ref(qg, kr[h], vh[h], kc[l], vc[l], btr, n, h, emulate)
                    if case.family == "needle":
                        out["needle_gap"] = min(out["needle_gap"], _lead(qg, kr[h], kc[l], btr, n, h))
                else:
                    o = _attend_emu(p, qg, kr[h], vh[h], inp.k_cache[sl], inp.v_cache[sl],
                                    inp.k_cache[l - 1] if l > 0 else None, inp.v_cache[l - 1] if l > 0 else None,
                                    btr, n, hr, m, applied)
                attn[b, h * gq * HD:(h + 1) * gq * HD] = o.reshape(-1)
            # the append (after the attention: this launch never reads it)
            wslot = slot
            if m == "append_slot_plus" and 0 <= slot < kc.shape[1] * KBS - 1:
                wslot, _ = slot + 1, applied.append(m)
            if m == "append_slot_minus" and slot >= 1:
                wslot, _ = slot - 1, applied.append(m)
            if m == "padding_row_writes" and slot < 0:
                wslot, _ = 15, applied.append(m)
            if wslot >= 0:
                blk, off = wslot // KBS, wslot % KBS
                kc[l, blk, :, off] = kr.to(BF)
                if m == "v_untransposed":
                    vc[l, blk].view(hkv, -1)[:, off * HD:(off + 1) * HD] = vh.to(BF)
                    applied.append(m)
                else:
                    vc[l, blk, :, :, off] = vh.to(BF)
        attn_r = attn if (p is None and not emulate) else rb(attn)
        o_upd = rb(_stream(p, "o", lw["wo"], rb(attn), mut, applied))
        res = res + o_upd
        x2 = _norm(res, lg["ln2"].double())
        gu = rb(_stream(p, "gu", lw["w13"], x2, mut, applied))
        g, u = gu[:, :I], gu[:, I:]
        if p is None:
            act = rb(g / (1.0 + torch.exp(-g)) * u)
        else:
            gf, uf = g.float(), u.float()
            act = rb(gf / (1.0 + torch.exp(-gf)) * uf)
            act = _pair_shift(p, "gu", act, applied) if m == "pair_shift" and mut.stream == "gu" else act
        if l == L - 1 and m == "hout_before_last_down":
            out["h_out"], _ = rb(res), applied.append(m)
        res = res + rb(_stream(p, "down", lw["w2"], act, mut, applied))
        out.update(qkv=qkv, attn=attn_r, act=act)
    out["res"] = res
    out.setdefault("h_out", rb(res))
    out["k_cache"], out["v_cache"] = kc, vc
    return out, applied


# ------------------------------------------------------------------------------------------------
# comparators


def appended(inp: Inputs):
    """(layer-independent) list of (b, block, offset) the step appends."""
    return [(b, int(s) // KBS, int(s) % KBS) for b, s in enumerate(inp.slot.tolist()) if s >= 0]


def check(inp: Inputs, got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], emulated: Optional[Dict] = None,
          stats: Optional[Dict] = None) -> float:
    """The family's comparators on everything the test observes.  got: what the kernel (or the
    emulation) left — qkv / attn / act / res [B, .], h_out, k_cache, v_cache.  want: the fp64
    reference.  emulated: the bf16-emulating reference (soft families).  Returns the largest
    kernel / emulated attention ratio (0 for the exact families)."""
    case = inp.case
    fam, B = case.family, case.B
    c = lambda t: t.detach().double().cpu()
    for key in ("qkv", "act", "res", "h_out"):
        g, w = c(got[key])[:B], c(want[key])[:B]
        assert torch.equal(g, w), f"{case.name}: {key} differs at {(g != w).nonzero()[:4].tolist()} " \
                                  f"(got {g[g != w][:4].tolist()}, want {w[g != w][:4].tolist()})"
    ratio = 0.0
    ga, wa = c(got["attn"])[:B], c(want["attn"])[:B]
    if fam == "needle":
        assert torch.equal(ga, wa), f"{case.name}: attn differs at {(ga != wa).nonzero()[:4].tolist()}"
    elif fam == "count":
        ap.assert_exact_to_ulp(ga, wa, f"{case.name} attn")
        if stats is not None:
            _farther(ga, wa, stats)
    else:
        shp = (B, case.geo.hq, HD)
        ratio = ap.assert_attention_close(ga.view(shp), wa.view(shp), c(emulated["attn"])[:B].view(shp), case.name)
    # the caches: bit-equal to the reference image (the inputs plus the appended entries); rope: the
    # appended K within one bf16 ulp of fp64, everything else bit-equal
    gk, gv, wk, wv = c(got["k_cache"]), c(got["v_cache"]), c(want["k_cache"]), c(want["v_cache"])
    if fam == "rope":
        wk64 = want["k_exact"]
        for b, blk, off in appended(inp):
            ap.assert_exact_to_ulp(gk[:, blk, :, off], wk64[:, blk, :, off], f"{case.name} appended K")
            if stats is not None:
                _farther(gk[:, blk, :, off], wk64[:, blk, :, off], stats)
            gk = gk.clone()
            gk[:, blk, :, off] = wk[:, blk, :, off]
    assert torch.equal(gk, wk), f"{case.name}: k_cache differs at {(gk != wk).nonzero()[:4].tolist()}"
    assert torch.equal(gv, wv), f"{case.name}: v_cache differs at {(gv != wv).nonzero()[:4].tolist()}"
    return ratio


def _farther(g, w, stats):
    """Count the elements that are not the bf16 nearest to the fp64 value (still within one ulp)."""
    stats["n"] = stats.get("n", 0) + g.numel()
    stats["farther"] = stats.get("farther", 0) + int((g != rb(w)).sum())


def expected(inp: Inputs):
    """(want, emulated) of a case; asserts the builder's promises on the fp64 reference."""
    case = inp.case
    want, _ = step(inp, "ref")
    emu = None
    if case.family == "needle":
        for key in ("qkv", "attn", "act", "res", "h_out"):
            v = want[key]
            assert torch.equal(rb(v), v), f"{case.name}: reference {key} is not bf16-representable"
            assert (v == v.round()).all() and v.abs().max() <= 256, f"{case.name}: reference {key} leaves the ledger"
        assert want["res"].abs().max() >= 1
        assert want["needle_gap"] >= 200, f"{case.name}: the needle leads by {want['needle_gap']:.0f} only"
    else:
        emu, _ = step(inp, "ref", emulate=True)
        for key in ("qkv", "act", "res", "h_out", "k_cache", "v_cache"):
            assert torch.equal(emu[key].double(), want[key].double())
    if case.family == "rope":     # the appended K without its bf16 rounding
        want["k_exact"] = _k_exact(inp, want)
    return want, emu


def _k_exact(inp: Inputs, want) -> torch.Tensor:
    geo = inp.case.geo
    kx = want["k_cache"].double().clone()
    assert inp.case.L == 1
    half = HD // 2
    for b, blk, off in appended(inp):
        k = want["qkv"][b, geo.hq * HD:(geo.hq + geo.hkv) * HD].view(geo.hkv, HD)
        cs = inp.cos_sin[int(inp.pos[b])].double()
        c, s = cs[:half], cs[half:]
        kx[0, blk, :, off] = torch.cat([k[:, :half] * c - k[:, half:] * s, k[:, half:] * c + k[:, :half] * s], dim=-1)
    return kx


# ------------------------------------------------------------------------------------------------
# mutations (the CPU self-test)

STREAM_MUTS = [Mut(n, s) for n in ("drop_chunk", "double_chunk", "stale_chunk", "rotate_x", "row_shift", "lose_last_row",
                                   "lose_last_row_partial", "swap_x_rows") for s in STREAMS] + \
              [Mut("lose_row63", s) for s in ("qkv", "o", "gu")] + \
              [Mut("swap_gate_up", "gu"), Mut("pair_shift", "qkv"), Mut("pair_shift", "gu"), Mut("leaders_get_o_rows", "o")]
ATTN_MUTS = [Mut(n) for n in ("lose_last_cached", "lose_chunk8", "lose_second_block", "ring_prev_layer", "next_kv_head",
                              "other_layer_slab", "other_seq_table", "other_seq_pos", "other_seq_ctx", "no_new_token",
                              "double_new_token", "mask_early", "mask_late", "append_slot_plus", "append_slot_minus",
                              "v_untransposed", "padding_row_writes", "poison_leak")]
MUTATIONS = STREAM_MUTS + ATTN_MUTS + [Mut(n) for n in LAYER_MUTS]


def mut_id(m: Mut) -> str:
    return m.name if m.stream is None else f"{m.name}-{m.stream}"


def same_outputs(a: Dict, b: Dict, B: int) -> bool:
    return all(torch.equal(torch.nan_to_num(a[k].double()[:B] if k not in ("k_cache", "v_cache") else a[k].double(), nan=-7e33),
                           torch.nan_to_num(b[k].double()[:B] if k not in ("k_cache", "v_cache") else b[k].double(), nan=-7e33))
               for k in ("qkv", "attn", "act", "res", "h_out", "k_cache", "v_cache"))


# ------------------------------------------------------------------------------------------------
# what the case list covers of the weight streams


ROW_CLASSES = ("rows 0", "rows 1", "rows odd", "rows 64", "partial last wave")
TOTAL_CLASSES = ("total < HB", "total = HB", "total = HB + 1", "total odd", "total >= 2 HB + 1")


def stream_classes(p: Part):
    """{(stream, HB, class)} a launch with this partition runs."""
    out = set()
    for s in STREAMS:
        cnt, hb, kc = p.counts(s), p.hb(s), p.kc(s)
        full = max(cnt)
        for n in set(cnt):
            tot = n * kc
            flags = (n == 0, n == 1, n > 1 and n % 2 == 1, n == 64, 0 < n < full,
                     0 < tot < hb, tot == hb, tot == hb + 1, tot % 2 == 1, tot >= 2 * hb + 1)
            out |= {(s, hb, k) for k, f in zip(ROW_CLASSES + TOTAL_CLASSES, flags) if f}
    return out


def unreachable(stream: str, hb: int, cls: str) -> bool:
    """(stream, HB, class) combinations no launch the host checks admit can run:
      HB 6 is the 12-slot down ring of B = 2 alone, HB 7 the 14-slot rings of B = 2 at GQA > 4 (never
        the down rows, which then have 12 slots);
      gate / up rows come in pairs: never 1 row, an odd count or an odd total (so neither 7 nor 9);
      64 down rows per wave would be more than 64 O rows (fewer workgroups share those): refused;
      64 QKV rows at HB 7: B = 2 needs 3 workgroups per KV group, at most ceil(1280 / 24) = 54 rows."""
    if hb == 6:
        return stream != "down" or cls == "rows 64"
    if hb == 7 and stream == "down":
        return True
    if stream == "down" and cls == "rows 64":
        return True
    if stream == "gu":
        if cls in ("rows 1", "rows odd", "total odd"):
            return True
        if (hb, cls) in ((8, "total = HB + 1"), (7, "total = HB")):
            return True
    return hb == 7 and (stream, cls) == ("qkv", "rows 64")


def build_random(case: Case) -> Inputs:
    """The same launch on random weights (randn / sqrt(K), gains near 1, randn caches): what the
    model tests feed the kernel.  For the self-test's demonstrations of what a loose tolerance on
    such inputs lets through."""
    inp = build(case)
    gen = torch.Generator().manual_seed(case.seed + 1)
    geo = case.geo
    rn = lambda *s: torch.randn(*s, generator=gen)
    inp.h0 = rn(case.B, geo.H).to(BF)
    for l in inp.layers:
        l["wqkv"] = (rn(geo.qkvn, geo.H) / geo.H ** 0.5).to(BF)
        l["wo"] = (rn(geo.H, geo.hq * HD) / (geo.hq * HD) ** 0.5).to(BF)
        l["w13"] = (rn(2 * geo.I, geo.H) / geo.H ** 0.5).to(BF)
        l["w2"] = (rn(geo.H, geo.I) / geo.I ** 0.5).to(BF)
        l["ln1"] = (1 + 0.1 * rn(geo.H)).to(BF)
        l["ln2"] = (1 + 0.1 * rn(geo.H)).to(BF)
    live = inp.k_cache != POISON
    inp.k_cache = torch.where(live, rn(*inp.k_cache.shape).to(BF), inp.k_cache)
    inp.v_cache = torch.where(inp.v_cache != POISON, rn(*inp.v_cache.shape).to(BF), inp.v_cache)
    inp.cos_sin = ref.rope_cos_sin(int(inp.pos.max()) + 2, HD, ap.ROPE_THETA)
    return inp
