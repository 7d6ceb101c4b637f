"""Constructed inputs with exactly known answers (or answers bounded by one bf16 ulp) for the kernels of
csrc/elementwise.hip (RMSNorm, RoPE + paged-KV append, SiLU*mul, embedding), csrc/sampling.hip (masked
argmax, router top-k) and the routing half of csrc/moe.hip (align, sort, combine); their fp64 or exact
references, comparators, the case lists shared by tests/test_elementwise_probes_cpu.py and
tests/test_elementwise_probes_gpu.py, and torch emulations of the kernels that can be broken on
purpose (`mut=`).  Importable without a GPU.

Tolerances, each derived here and none fitted to a kernel's output:

RoPE, exact family.  qkv holds integers in [-8, 8], the table multiples of 1/4 in [-2, 2]; x1 c - x2 s
is then a multiple of 1/4 of magnitude <= 32, i.e. n / 4 with |n| <= 128: eight significant bits, exact
in fp32 with or without FMA contraction and exact in bf16.  Compared with torch.equal.
RoPE, real table.  |got - want| <= 2^-8 |want| + 2^-20 (|x1| + |x2|): bf16 rounding of an fp32 result
(half an ulp is at most 2^-8 of the value) plus the fp32 arithmetic under cancellation (two products and
a sum, each within 2^-24 of operands bounded by |x1| + |x2| since |cos|, |sin| <= 1; 2^-20 leaves 5x).

RMSNorm.  |got - want| <= 2^-8 |want| against fp64: one bf16 rounding of an fp32 value that is a few
fp32 ulp (rsqrtf, summation order) from the truth.  A value that the fp32 error carries across a
rounding boundary lies >= 2^-8 above its binade's start, which leaves 2^-16 |want| of slack against an
fp32 error of ~2^-22.  No probed output is zero, so no absolute term.  The residual written back equals
bf16(x + res) exactly: one fp32 add of two bf16 values, one rounding.

SiLU*mul.  One bf16 ulp of the fp64 answer, plus SILU_FLOOR = 2^-119.  The kernel computes
g / (1 + exp(-g)) in fp32; exp(-g) overflows fp32 for -g > ln(FLT_MAX) = 88.7228, and the kernel then
returns -0 where the truth is |g| e^g <= 88.7228 / 3.4028e38 = 2.61e-37, times max |up| = 3: 7.82e-37 <
2^-119 = 1.50e-36.  The same floor covers results below the smallest normal fp32 (2^-126), which the
hardware may flush.  Above the floor the fp32 formula is within SILU_FP32_REL = 2^-16 of the fp64 value
(asserted on a CPU emulation): under 1 % of a bf16 ulp, so the rounded result is the fp64 answer's
nearest bf16 value or its neighbour, never two away.

Embedding, masked argmax (index and value), MoE align / sort / combine: exact.  Combine is exact because
Y holds integers in [-5, 5], the weights are powers of two in [1/4, 1] and k <= 4: every partial sum is a
multiple of 1/4 of magnitude <= 20.  Router top-k: ids exact, weights within 1e-5 (absolute) of the fp64
softmax renormalised over the winners, the tolerance of the older test: fp32 exp and three divisions
on values <= 1 stay below 1e-6.

Split-K slices are integers: slice k >= 1 is (-1)^k u with u in {1, 2} (non-zero everywhere, partial
sums bounded), slice 0 is the target minus the rest and non-zero in every 8-vector, so a dropped or
doubled slice changes every 16-byte vector of the sum and fp32 addition is exact in any order.
"""
from __future__ import annotations

import functools

import torch

BF = torch.bfloat16
SENT = 1000.0                  # bf16-exact; larger than any probed output
PAD = 3                        # sentinel rows around an out= view
SILU_FLOOR = 2.0 ** -119
SILU_FP32_REL = 2.0 ** -16
EPS = 1e-5


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def case_seed(*key) -> int:
    h = 0x2545F491
    for k in key:
        h = (h * 1000003 + int(k) + 0x7F4A7C15) % (2 ** 31 - 1)
    return h


def framed(rows: int, cols: int, device, dtype=BF):
    """(whole, view): `view` is the contiguous [rows, cols] interior of a sentinel-filled buffer."""
    whole = torch.full((rows + 2 * PAD, cols), SENT, dtype=dtype, device=device)
    return whole, whole[PAD:PAD + rows]


def assert_frame(whole: torch.Tensor, what: str) -> None:
    edge = torch.cat([whole[:PAD], whole[-PAD:]])
    assert bool((edge == SENT).all()), f"{what}: rows outside the out= view were written"


def int_slices(S: torch.Tensor, split: int, seed: int):
    """(P [split, *S.shape] fp32, S'): integer slices that sum to S' exactly, S' = S except where an
    8-vector of slice 0 would be all zero (its first element is moved by one: away from zero below 8,
    towards it from there)."""
    assert S.shape[-1] % 8 == 0
    g = _gen(seed)
    rest = torch.randint(1, 3, (split - 1, *S.shape), generator=g).float()
    sign = torch.tensor([(-1.0) ** k for k in range(1, split)]).reshape(-1, *([1] * S.dim()))
    rest = rest * sign
    S = S.float().clone()
    s0 = S - rest.sum(0)
    z = (s0.reshape(-1, 8) == 0).all(1)
    if bool(z.any()):
        S8 = S.view(-1, 8)
        f = S8[z, 0]
        S8[z, 0] = f + torch.where(f.abs() >= 8, -torch.sign(f), torch.where(f < 0, -1.0, 1.0))
        s0 = S - rest.sum(0)
    P = torch.cat([s0[None], rest]) if split > 1 else s0[None]
    assert bool((P.reshape(split, -1, 8) != 0).any(2).all()) and float(P.abs().max()) < 256
    assert torch.equal(P.sum(0), S)
    return P, S


def sum_slices(P: torch.Tensor, mut=None) -> torch.Tensor:
    """fp32 sum in slice order; slice_drop / slice_double hit the last slice (the one a wrong loop
    bound or `k0 + k < split` guard loses) ."""
    s = P.float().sum(0)
    if mut == "slice_drop":
        s = s - P[-1].float()
    elif mut == "slice_double":
        s = s + P[-1].float()
    return s


def assert_rel(got: torch.Tensor, want: torch.Tensor, rel: float, what: str, extra=None) -> None:
    got, want = got.double(), want.double().to(got.device)
    bound = rel * want.abs() + (0.0 if extra is None else extra.double().to(got.device))
    bad = ~((got - want).abs() <= bound)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, first at {i}: "
                             f"got {float(got[i])!r} want {float(want[i])!r}")


def assert_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    want = want.to(got.device)
    if got.dtype != want.dtype:
        got, want = got.double(), want.double()
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: "
                             f"got {float(got[i])!r} want {float(want[i])!r}")


# ====================================================================================================
# RoPE + paged-KV append
# ====================================================================================================
ROPE_MAX_POS = 64
ROPE_HEADS = ((4, 1), (8, 8), (32, 8))
ROPE_SPLITS = (1, 2, 4, 5, 8, 9)
ROPE_MUTATIONS = ("row_next_hi", "cos_sin_swap", "sin_sign", "group_reuse", "k_neighbour", "v_transposed",
                  "pad_written", "clamp_written", "slice_drop", "slice_double")
_WINDOW_KINDS = ("inblock", "straddle", "desc", "pad_first", "pad_window")


def rope_is_window(T: int, d: int, bs: int) -> bool:
    """csrc/elementwise.hip rope_window_ok with the default threshold."""
    return T >= 64 and d == 128 and bs == 16


def rope_cases():
    """dicts: T, hq, hkv, d, bs, rot (which slot pattern each 16-token window gets), pad_last, all_pad,
    split (0: bf16 qkv), real (the cos/sin table of ops.reference.rope_cos_sin and randn qkv)."""
    out = []

    def add(T, heads, d=128, bs=16, rot=0, pad_last=False, all_pad=False, split=0, real=False):
        out.append(dict(T=T, hq=heads[0], hkv=heads[1], d=d, bs=bs, rot=rot, pad_last=pad_last, all_pad=all_pad,
                        split=split, real=real))
    for heads in ROPE_HEADS:
        for T in (64, 65, 80, 95):                         # window kernel
            for rot in (0, 2):
                add(T, heads, rot=rot, pad_last=rot == 2)
        for T in (1, 15, 17, 63):                          # per-token kernel
            add(T, heads, rot=0, pad_last=T == 15)
            add(T, heads, rot=3, pad_last=T == 63)
        add(80, heads, d=64)                               # per-token kernel at T >= 64
        add(80, heads, bs=32, rot=1)
    for T in (80, 17):
        add(T, (8, 8), all_pad=True)
        add(T, (8, 8), real=True)
        for split in ROPE_SPLITS:
            add(T, (4, 1), split=split, rot=1, pad_last=split == 5)
            add(T, (8, 8), split=split, rot=4)
    add(95, (8, 8), split=5, real=True)
    return out


def rope_exact_table(d: int, max_pos: int = ROPE_MAX_POS) -> torch.Tensor:
    """[max_pos, d] fp32, cos | sin, multiples of 1/4 in [-2, 2].  With a = 3 pos + 5 i + i // 4: neighbouring
    positions differ in every pair (3), cos != sin (7), and pair i differs from pair i + 4 of the same
    8-pair chunk (21 = 4), all modulo 17."""
    half = d // 2
    p = torch.arange(max_pos)[:, None]
    i = torch.arange(half)[None, :]
    a = 3 * p + 5 * i + i // 4
    return torch.cat([(a % 17 - 8) / 4.0, ((a + 7) % 17 - 8) / 4.0], 1).float()


def rope_slots(T: int, bs: int, rot: int, pad_last: bool, all_pad: bool):
    """(slots int32 [T], NB).  Window w owns blocks 1 + 4w and 3 + 4w (not adjacent); block 0 and slot 0
    are never used, so a padding token that is written anyway lands on a sentinel."""
    nwin = (T + 15) // 16
    slots = torch.full((T,), -1, dtype=torch.int32)
    if not all_pad:
        for w in range(nwin):
            kind = _WINDOW_KINDS[(w + rot) % len(_WINDOW_KINDS)]
            A, B = (1 + 4 * w) * bs, (3 + 4 * w) * bs
            nt = min(16, T - 16 * w)
            if nt < 16 and kind == "pad_window":
                kind = "inblock"                           # the partial last window keeps valid tokens
            for j in range(nt):
                s = {"inblock": A + j, "straddle": A + bs - 8 + j if j < 8 else B + j - 8, "desc": A + 15 - j,
                     "pad_first": A + j if j else -1, "pad_window": -1}[kind]
                slots[16 * w + j] = s
        if pad_last:
            slots[T - 1] = -1
    return slots, 4 * nwin + 2


@functools.lru_cache(maxsize=2)
def _rope_build(key):
    c = dict(key)
    T, hq, hkv, d, bs = c["T"], c["hq"], c["hkv"], c["d"], c["bs"]
    W = (hq + 2 * hkv) * d
    g = _gen(case_seed(T, hq, hkv, d, bs, c["rot"], c["split"]))
    slots, NB = rope_slots(T, bs, c["rot"], c["pad_last"], c["all_pad"])
    if c["real"]:
        from ai_agent_kubectl_amd.ops import reference as ref
        table = ref.rope_cos_sin(4096, d, 5e5)
        pos = torch.randint(0, 4096, (T,), generator=g).int()
        x = torch.randn(T, W, generator=g).to(BF).float()
        if c["split"]:
            x = torch.randint(-8, 9, (T, W), generator=g).float()
    else:
        table = rope_exact_table(d)
        pos = ((torch.arange(T) * 7 + 3) % ROPE_MAX_POS).int()
        x = torch.randint(-8, 9, (T, W), generator=g).float()
    pos[0] = 0
    pos[T // 2] = table.shape[0] - 1
    P = None
    if c["split"]:
        P, x = int_slices(x, c["split"], case_seed(T, W, c["split"]))
        assert float(x.abs().max()) <= 8
    return dict(c, x=x.to(BF), P=P, pos=pos, table=table, slots=slots, NB=NB)


def rope_inputs(case):
    """The case plus x (bf16 qkv), P (fp32 slices or None), pos, table, slots, NB; cached: leave unchanged."""
    return _rope_build(tuple(sorted(case.items())))


def rope_caches(c, device="cpu"):
    k = torch.full((c["NB"], c["hkv"], c["bs"], c["d"]), SENT, dtype=BF, device=device)
    v = torch.full((c["NB"], c["hkv"], c["d"], c["bs"]), SENT, dtype=BF, device=device)
    return k, v


def _rope_core(c, x, table, dtype, mut=None):
    """(q [T, hq, d], kc, vc, magnitudes) in `dtype`; caches start from SENT.  fp64: the reference."""
    T, hq, hkv, d, bs = c["T"], c["hq"], c["hkv"], c["d"], c["bs"]
    half = d // 2
    pos, slots = c["pos"].long(), c["slots"].long()
    x = x.to(dtype)
    cs = table.to(dtype)[pos]
    cos, sin = cs[:, :half].clone(), cs[:, half:].clone()
    if mut == "row_next_hi":
        nx = table.to(dtype)[(pos + 1) % table.shape[0]]
        cos[:, 32:], sin[:, 32:] = nx[:, 32:half], nx[:, half + 32:]
    elif mut == "cos_sin_swap":
        cos, sin = sin, cos
    elif mut == "sin_sign":
        sin = -sin
    elif mut == "group_reuse":
        i = torch.arange(half)
        i = torch.where(i % 8 >= 4, i - 4, i)
        cos, sin = cos[:, i], sin[:, i]
    qk = x[:, :(hq + hkv) * d].view(T, hq + hkv, d)
    x1, x2 = qk[..., :half], qk[..., half:]
    co, si = cos[:, None], sin[:, None]
    rot = torch.cat([x1 * co - x2 * si, x2 * co + x1 * si], -1)
    mag = (x1.abs() + x2.abs()).repeat(1, 1, 2)
    v = x[:, (hq + hkv) * d:].view(T, hkv, d)
    kc = torch.full((c["NB"], hkv, bs, d), SENT, dtype=dtype)
    vc = torch.full((c["NB"], hkv, d, bs), SENT, dtype=dtype)
    kmag = torch.zeros_like(kc)
    valid = (slots >= 0).nonzero().squeeze(1)
    kslots = slots.clone()
    if mut == "k_neighbour":
        kslots[valid] = slots[valid.roll(-1)]
    if mut == "pad_written":
        slots = slots.clamp(min=0)
        kslots = kslots.clamp(min=0)
        valid = torch.arange(T)
    for t in valid.tolist():
        kb, ko = divmod(int(kslots[t]), bs)
        kc[kb, :, ko, :] = rot[t, hq:]
        kmag[kb, :, ko, :] = mag[t, hq:]
        b, o = divmod(int(slots[t]), bs)
        if mut == "v_transposed":
            vc[b].view(hkv, bs, d)[:, o, :] = v[t]
        else:
            vc[b, :, :, o] = v[t]
    if mut == "clamp_written":
        b, o = divmod(int(slots[T - 1]), bs)
        vc[b, :, :, o] = 0
    return rot[:, :hq].contiguous(), kc, vc, mag[:, :hq].contiguous(), kmag


def rope_want(c):
    """fp64 reference: (q, kc, vc, q_mag, k_mag); unwritten cache elements hold SENT (k_mag 0 there)."""
    return _rope_core(c, c["x"], c["table"], torch.float64)


def rope_mutation_applies(mut: str, c) -> bool:
    nvalid = int((c["slots"] >= 0).sum())
    if mut == "row_next_hi":
        return c["d"] // 2 > 32
    if mut in ("k_neighbour",):
        return nvalid >= 2
    if mut == "v_transposed":
        return nvalid >= 1
    if mut == "pad_written":
        return nvalid < c["T"]
    if mut == "clamp_written":
        return rope_is_window(c["T"], c["d"], c["bs"]) and c["T"] % 16 != 0 and int(c["slots"][-1]) >= 0
    if mut in ("slice_drop", "slice_double"):
        return c["split"] >= 1
    return True


def rope_emulate(c, mut=None):
    """The kernels' arithmetic in fp32 on the bf16(-rounded sum of the) input: (q, kc, vc) bf16."""
    x = sum_slices(c["P"], mut).to(BF) if c["P"] is not None else c["x"]
    q, kc, vc, _, _ = _rope_core(c, x.float(), c["table"], torch.float32, mut)
    return q.to(BF), kc.to(BF), vc.to(BF)


def assert_rope(c, q, kc, vc, want, what: str) -> None:
    wq, wk, wv, qm, km = want
    q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()
    if not c["real"]:
        assert_equal(q, wq.to(BF), f"{what}: q_out")
        assert_equal(kc, wk.to(BF), f"{what}: k_cache")
    else:
        assert_rel(q, wq, 2.0 ** -8, f"{what}: q_out", 2.0 ** -20 * qm)
        written = wk != SENT                               # unwritten elements: exactly the sentinel (bound 0)
        assert_rel(kc, wk, 2.0 ** -8, f"{what}: k_cache", 2.0 ** -20 * km - 2.0 ** -8 * SENT * (~written))
    assert_equal(vc, wv.to(BF), f"{what}: v_cache")


# ====================================================================================================
# RMSNorm
# ====================================================================================================
RMS_MUTATIONS = ("vec_lost", "wave_lost", "padded_mean", "eps_dropped", "res_unrounded", "slice_drop",
                 "slice_double")
RMS_BIG = 64.0          # the probed element; the rest of the row is 2^-6
RMS_BIG_INT = 128.0     # split-K rows are integers: +-1 everywhere, +-128 at the probed element


def rms_variant(rows: int, hidden: int, splitk: bool):
    """(NT, MAXV, UNR) of the rmsnorm_kernel instance ka_rmsnorm / launch_rmsnorm_splitk launch."""
    nvec = hidden // 8
    if nvec <= 256:
        nt, mv = 256, 1
    elif splitk:
        nt, mv = (512, 1) if nvec <= 512 else (512, 2) if rows <= 1024 else (256, 4)
    elif nvec <= 512:
        nt, mv = (512, 1) if rows <= 1024 else (256, 2)
    else:
        nt, mv = 256, 4
    unr = (8 if nt >= 512 else 4) if mv == 1 else 4 if mv == 2 else 2
    return nt, mv, unr


def rms_probe_positions(hidden: int, nt: int, mv: int):
    """First and last element of every thread-slot boundary, and one element of every wave."""
    p = {0, 7, 8, hidden - 8, hidden - 1}
    for i in range(1, mv + 1):
        p |= {i * nt * 8 - 1, i * nt * 8, i * nt * 8 + 7}
    for i in range(mv):
        for w in range(nt // 64):
            p.add((i * nt + 64 * w + 17) * 8 + 3)
    return sorted(q for q in p if 0 <= q < hidden)


RMS_HIDDENS = (8, 2048, 2056, 4096, 4104, 8192)


def rms_cases():
    """(rows, hidden, split, p_bf16); split 0: the bf16 entry point.  rows 0 = one row per probe + the eps row."""
    out = [(0, h, 0, False) for h in RMS_HIDDENS] + [(1025, 4096, 0, False), (1025, 8192, 0, False)]
    shapes = [(0, h) for h in RMS_HIDDENS] + [(1025, 8192)]
    for rows, h in shapes:
        unr = rms_variant(rows or 1, h, True)[2]
        for split in (unr - 1, unr, unr + 1, 2 * unr, 2 * unr + 1):
            for pb in (False, True):
                out.append((rows, h, split, pb))
    out += [(1025, 4096, 9, False), (1025, 4096, 9, True)]
    return out


def rms_weight(hidden: int) -> torch.Tensor:
    i = torch.arange(hidden)
    return (0.5 + 0.25 * ((i + i // 8) % 6)).to(BF)


@functools.lru_cache(maxsize=2)
def rms_inputs(rows: int, hidden: int, split: int, p_bf16: bool):
    """dict: x bf16 [rows, hidden] (the sum of P when split), P, res bf16, w, probes, variant.  Row r probes
    position probes[r % (n + 1)]; index n is the eps row (2^-10 everywhere; integers cannot do that, so
    under split-K it is a row of +-1 without a probed element)."""
    nrows = rows or 1
    nt, mv, unr = rms_variant(nrows, hidden, split > 0)
    probes = rms_probe_positions(hidden, nt, mv)
    n = len(probes)
    rows = rows or n + 1
    g = _gen(case_seed(rows, hidden, split))
    r = torch.arange(rows)
    which = r % (n + 1)
    if split:
        x = (torch.randint(0, 2, (rows, hidden), generator=g) * 2 - 1).float()
        hit = which < n
        pp = torch.tensor(probes + [0])[which]
        x[r[hit], pp[hit]] *= RMS_BIG_INT
        P, x = int_slices(x, split, case_seed(rows, hidden, split, 1))
        x = x.to(BF)
        res = (torch.randn(rows, hidden, generator=g) * 0.5).clamp(-0.9, 0.9).to(BF)    # |x + res| >= 0.1
        if p_bf16:
            P = P.to(BF)
    else:
        row = torch.full((rows, hidden), 2.0 ** -6)
        hit = which < n
        pp = torch.tensor(probes + [0])[which]
        row[r[hit], pp[hit]] = RMS_BIG
        row[~hit] = 2.0 ** -10
        P = None
        x = row.to(BF)
        res = (torch.randn(rows, hidden, generator=g) * 0.5).clamp(-1.9, 1.9).to(BF)
        res[~hit] = 0
    return dict(rows=rows, hidden=hidden, split=split, x=x, P=P, res=res, w=rms_weight(hidden), probes=probes,
                variant=(nt, mv, unr))


def rms_x_for_residual(c) -> torch.Tensor:
    """x with x + res close to the probe rows (bf16 entry point only): the residual add then rounds."""
    return (c["x"].float() - c["res"].float()).to(BF)


def rms_want(x: torch.Tensor, w: torch.Tensor, res=None):
    """fp64 on x's device: (out, residual bf16 or None)."""
    r = None
    if res is not None:
        r = (x.float() + res.float()).to(BF)
        x = r
    xd = x.double()
    return xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS) * w.double().to(x.device), r


def rms_mutation_applies(mut: str, c, with_res: bool) -> bool:
    nt, mv, _ = c["variant"]
    if mut == "padded_mean":
        return nt * mv * 8 != c["hidden"]
    if mut == "eps_dropped":
        return c["split"] == 0
    if mut == "res_unrounded":
        return with_res
    if mut == "slice_drop":
        return c["split"] > 0
    if mut == "slice_double":                              # doubling the only slice scales the row: the norm is unchanged
        return c["split"] > 1 or (c["split"] == 1 and with_res)
    return True


def _trunc_bf16(t: torch.Tensor) -> torch.Tensor:
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def rms_emulate(c, x: torch.Tensor, with_res: bool, mut=None):
    """The kernel in fp32: (out bf16, residual bf16 or None)."""
    nt, mv, _ = c["variant"]
    hidden = c["hidden"]
    if c["P"] is not None:
        x = sum_slices(c["P"], mut).to(BF)
    v = x.float()
    r = None
    if with_res:
        s = v + c["res"].float()
        r = s.to(BF)
        v = r.float()
        if mut == "res_unrounded":
            r, v = _trunc_bf16(s), s
    sq = (v * v).view(v.shape[0], hidden // 8, 8).sum(2)
    nvec = hidden // 8
    if mut == "vec_lost":
        sq[:, nvec - 1] = 0
    elif mut == "wave_lost":
        idx = torch.arange(nvec)
        sq[:, (idx % nt) // 64 == ((nvec - 1) % nt) // 64] = 0
    tot = sq.sum(1, keepdim=True)
    mean = tot / (nt * mv * 8 if mut == "padded_mean" else hidden)
    scale = torch.rsqrt(mean + (0.0 if mut == "eps_dropped" else EPS))
    return (v * scale * c["w"].float()).to(BF), r


# ====================================================================================================
# SiLU * mul, embedding
# ====================================================================================================
SILU_UPS = (1.0, -3.0, 0.5)
SILU_SPLITS = (1, 2, 4, 5, 8, 9, 16)
SILU_GRID = (2049, 4096)       # 1,049,088 vectors: 512 more than 4096 blocks x 256 threads
SILU_GRID_CAP = 4096 * 256
SILU_MUTATIONS = ("gate_up_swap", "sigmoid", "scaled", "second_pass_skipped", "slice_drop", "slice_double")


@functools.lru_cache(maxsize=1)
def silu_exhaustive() -> torch.Tensor:
    """gu [3, 2 * 65536] bf16: every finite bf16 bit pattern as the gate (the 256 non-finite ones replaced
    by 1.0), up = 1, -3, 0.5 per row."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32)
    bits = torch.where((bits & 0x7F80) == 0x7F80, torch.tensor(0x3F80, dtype=torch.int32), bits)
    gate = bits.to(torch.int16).view(BF)
    assert bool(torch.isfinite(gate.float()).all()) and gate.unique().numel() >= 65536 - 256 - 1
    up = torch.tensor(SILU_UPS)[:, None].expand(3, 65536).to(BF)
    return torch.cat([gate[None].expand(3, -1), up], 1).contiguous()


def silu_grid_input(device="cpu") -> torch.Tensor:
    """gu [2049, 8192]: integer gate in [-8, 8] and non-zero integer up in [-6, 6], different in every row
    and every 8-vector."""
    T, I = SILU_GRID
    t = torch.arange(T, device=device)[:, None]
    c = torch.arange(I, device=device)[None, :]
    gate = (t * 7 + c * 3 + c // 8) % 17 - 8
    up = (t * 5 + c + 3 * (c // 8)) % 12 - 6
    up = torch.where(up >= 0, up + 1, up)
    return torch.cat([gate, up], 1).to(BF)


@functools.lru_cache(maxsize=8)
def silu_split_input(split: int, T: int = 5, I: int = 64):
    g = _gen(case_seed(split, T, I))
    S = torch.randint(-8, 9, (T, 2 * I), generator=g).float()
    P, S = int_slices(S, split, case_seed(split, T, I, 1))
    return P, S.to(BF)


def silu_want(gu: torch.Tensor) -> torch.Tensor:
    I = gu.shape[1] // 2
    g, u = gu[:, :I].double(), gu[:, I:].double()
    return g / (1.0 + torch.exp(-g)) * u


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 values at |v| (fp64): 2^(floor(log2 |v|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 7)


BF16_MAX = float.fromhex("0x1.fcp127")     # the largest finite bf16


def assert_silu(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """One bf16 ulp of the fp64 answer plus SILU_FLOOR.  Where the fp64 answer is past the largest finite
    bf16 (gates above 1.13e38 times up = -3) the rounded answer is that value or the infinity of its sign."""
    want = want.to(got.device)
    g = got.double()
    ok = (g - want).abs() <= bf16_ulp(want) + SILU_FLOOR
    ok |= (want.abs() > BF16_MAX) & (g == torch.sign(want) * float("inf"))
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, first at {i}: "
                             f"got {float(g[i])!r} want {float(want[i])!r}")


def silu_emulate_fp32(gu: torch.Tensor, mut=None) -> torch.Tensor:
    """The kernel's formula in fp32, before the bf16 rounding."""
    I = gu.shape[1] // 2
    g, u = gu[:, :I].float(), gu[:, I:].float()
    if mut == "gate_up_swap":
        g, u = u, g
    s = 1.0 / (1.0 + torch.exp(-g)) if mut == "sigmoid" else g / (1.0 + torch.exp(-g))
    return s * u * (1.015 if mut == "scaled" else 1.0)


def silu_emulate(gu: torch.Tensor, mut=None, P=None) -> torch.Tensor:
    if P is not None:
        gu = sum_slices(P, mut).to(BF)
    out = silu_emulate_fp32(gu, mut).to(BF)
    if mut == "second_pass_skipped":
        flat = out.view(-1, 8)
        flat[SILU_GRID_CAP:] = SENT
    return out


EMB_OFFSETS = (0, 8, 1000)
EMB_HIDDENS = (8, 2048, 2056)
EMB_VOCAB = 50
EMB_MUTATIONS = ("offset_ignored", "last_row_refused", "tail_skipped")


def emb_inputs(hidden: int, off: int):
    g = _gen(case_seed(hidden, off))
    table = torch.randint(1, 100, (EMB_VOCAB, hidden), generator=g).to(BF)
    ids = torch.tensor([off - 1, off, off + EMB_VOCAB - 1, off + EMB_VOCAB, -1, -7, off + 17, off + 1, off + EMB_VOCAB + 9],
                       dtype=torch.int32)
    return table, ids


def emb_want(table: torch.Tensor, ids: torch.Tensor, off: int, mut=None) -> torch.Tensor:
    V = table.shape[0]
    loc = ids.long() - (0 if mut == "offset_ignored" else off)
    ok = (loc >= 0) & (loc < (V - 1 if mut == "last_row_refused" else V))
    out = table[loc.clamp(0, V - 1)] * ok[:, None].to(table.dtype)
    if mut == "tail_skipped" and table.shape[1] > 2048:
        out[:, 2048:] = SENT
    return out


# ====================================================================================================
# Masked argmax
# ====================================================================================================
ARGMAX_BS = (1, 127, 128)
ARGMAX_VS = (8, 4096, 32768 + 8, 128256)
ARGMAX_OFFS = (0, 8, 24, 64)
ARGMAX_MUTATIONS = ("mask_shift", "mask_local", "tie_highest", "slice_tail_skipped")
ARGMAX_NT = 512


def argmax_slices(B: int, V: int) -> int:
    """csrc/sampling.hip ka_argmax_slices (the GPU module checks this against the library)."""
    if B >= 128:
        return 1
    s = 1
    while s < 64 and B * s * 2 <= 512 and V // (s * 2) >= 4096:
        s *= 2
    return s


def argmax_slice_bounds(V: int, slices: int):
    nvec = V // 8
    per = -(-nvec // slices)
    return [(min(nvec, j * per) * 8, min(nvec, (j + 1) * per) * 8) for j in range(slices)]


def argmax_cases():
    return [(B, V, off) for B in ARGMAX_BS for V in ARGMAX_VS for off in ARGMAX_OFFS]


@functools.lru_cache(maxsize=2)
def argmax_inputs(B: int, V: int, off: int):
    """dict: logits bf16 [n, V], bits int32 [n, words] (indexed by the global id), midx int32 [n], rows
    (the spec of each row), slices.  n = B, or every probe row when B = 1 (the GPU module then calls once
    per row).  A probe row: background -1 .. -7, 10 at the probed position, 20 on a neighbour whose mask
    bit is clear."""
    slices = argmax_slices(B, V)
    pos = {0, 7, 8, V - 8, V - 1}
    for a, _ in argmax_slice_bounds(V, slices)[1:]:
        pos |= {a - 1, a}
    for b in (ARGMAX_NT * 8, ARGMAX_NT * 8 * 8):
        pos |= {b - 1, b}
    for m in (1, 2, V // 64, (V + off) // 32 - 1):          # both sides of a 32-bit mask word boundary
        pos |= {32 * m - off - 1, 32 * m - off}
    pos = sorted(p for p in pos if 0 <= p < V)
    rows = []
    for p in pos:
        for n in (p + 1, p - 1):
            if 0 <= n < V:
                rows.append(("probe", (p,), (n,)))
    lane = 5
    ties = [q for q in (lane, lane + 1, lane + 8, lane + 512, lane + ARGMAX_NT * 8, lane + ARGMAX_NT * 64) if q < V]
    sb = [a + lane for a, _ in argmax_slice_bounds(V, slices)[1:] if a + lane < V]
    ties = sorted(set(ties + sb))
    rows.append(("tie", tuple(ties), ()))
    rows.append(("tie_unmasked", tuple(ties), ()))
    for i in range(len(ties) - 1):
        rows.append(("tie", (ties[i], ties[i + 1]), ()))
    if len(ties) > 1:
        rows.append(("tie", tuple(ties), (ties[0],)))          # the lowest copy is masked out
    rows.append(("all_masked", (), ()))
    if B > 1:
        assert len(rows) <= B, (len(rows), B)
        rows = [rows[i % len(rows)] for i in range(B)]
    n = len(rows)
    words = (V + off + 31) // 32
    i = torch.arange(V)
    logits = (-1.0 - (i % 7)).repeat(n, 1)
    bits = torch.full((n, words), -1, dtype=torch.int32)
    midx = torch.arange(n, dtype=torch.int32)
    for r, (kind, hot, masked) in enumerate(rows):
        for p in hot:
            logits[r, p] = 10.0
        for m in masked:
            if kind == "probe":
                logits[r, m] = 20.0
            gb = m + off
            bits[r, gb // 32] &= ~(1 << (gb % 32)) if gb % 32 < 31 else 0x7FFFFFFF
        if kind == "all_masked":
            bits[r] = 0
        if kind == "tie_unmasked":
            midx[r] = -1
    return dict(B=B, V=V, off=off, logits=logits.to(BF), bits=bits, midx=midx, rows=rows, slices=slices)


def argmax_allowed(bits: torch.Tensor, midx: torch.Tensor, V: int, off: int, mut=None) -> torch.Tensor:
    gid = torch.arange(V) + (0 if mut == "mask_local" else off) + (1 if mut == "mask_shift" else 0)
    word = bits[:, (gid // 32).clamp(max=bits.shape[1] - 1)].long() & 0xFFFFFFFF
    allowed = ((word >> (gid % 32)) & 1).bool()
    return allowed | (midx < 0)[:, None]


def argmax_pick(c, mut=None):
    """(global id int32 [n], value fp32 [n]).  mut None: the expected answer (lowest allowed id among the
    row's maxima; a fully masked row gives off + 0 and -inf)."""
    V, off = c["V"], c["off"]
    allowed = argmax_allowed(c["bits"], c["midx"], V, off, mut)
    if mut == "slice_tail_skipped":
        for _, b in argmax_slice_bounds(V, c["slices"]):
            allowed[:, b - 8:b] = False
    lf = c["logits"].float().masked_fill(~allowed, float("-inf"))
    val = lf.max(1).values
    hit = (lf == val[:, None]) & allowed
    i = torch.arange(V)
    if mut == "tie_highest":
        idx = torch.where(hit, i, -1).max(1).values.clamp(min=0)
    else:
        idx = torch.where(hit, i, V).min(1).values
        idx = torch.where(idx == V, 0, idx)
    return (idx + off).int(), val


def assert_argmax(idx, val, want_idx, want_val, what: str) -> None:
    idx, val = idx.cpu().int(), val.cpu().float()
    bad = (idx != want_idx) | (val != want_val)
    if bool(bad.any()):
        r = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} rows differ, first row {r}: got ({int(idx[r])}, {float(val[r])}) "
                             f"want ({int(want_idx[r])}, {float(want_val[r])})")


# ====================================================================================================
# Router top-k
# ====================================================================================================
TOPK_ES = (4, 8, 16, 64)
TOPK_TS = (1, 255, 256, 257)
TOPK_MUTATIONS = ("weights_swapped", "tie_highest", "no_renorm", "last_expert_ignored")


def topk_cases():
    return [(T, E, k) for E in TOPK_ES for k in sorted({1, 2, 4, E}) for T in TOPK_TS]


@functools.lru_cache(maxsize=4)
def topk_logits(T: int, E: int, k: int) -> torch.Tensor:
    """bf16 [T, E] within +-40.  Row t % 4 == 0: min(k - 1, E - 2) distinct leaders (the last expert first,
    then odd, then even ids) above a background of equal logits, so the last place (the last two at k = E)
    is a tie; 1: all equal; 2: multiples of 1/2 in [-6, 6] (ties everywhere); 3: distinct values spread
    over +-40 with the maximum on the last expert.  (T = 1 has row 0 only: at k = 1 it is all equal.)"""
    g = _gen(case_seed(T, E, k))
    lg = torch.randint(-12, 13, (T, E), generator=g).float() / 2
    t = torch.arange(T)
    lg[t % 4 == 1] = 1.5
    wide = ((torch.rand(T, E, generator=g).argsort(1).float() - (E - 1) / 2) * (80.0 / E)).to(BF).float()
    top = wide.argmax(1)
    last = wide[:, E - 1].clone()
    wide[:, E - 1] = wide[t, top]
    wide[t, top] = torch.where(top == E - 1, wide[:, E - 1], last)
    lg[t % 4 == 3] = wide[t % 4 == 3]
    tie = torch.full((E,), -3.0)
    order = [E - 1] + list(range(1, E - 1, 2)) + list(range(0, E - 1, 2))
    for j, e in enumerate(order[:min(k - 1, E - 2)]):
        tie[e] = 4.0 + 0.5 * j
    lg[t % 4 == 0] = tie
    assert float(lg.abs().max()) <= 40 and torch.equal(lg.to(BF).float(), lg)
    return lg.to(BF)


def topk_want(lg: torch.Tensor, k: int):
    """(weights fp64 [T, k], ids int32 [T, k]): stable descending sort of the bf16 logits (ties to the lower
    id), fp64 softmax renormalised over the winners."""
    ld = lg.double()
    ids = torch.sort(ld, dim=1, descending=True, stable=True).indices[:, :k]
    p = torch.softmax(ld, 1).gather(1, ids)
    return p / p.sum(1, keepdim=True), ids.int()


def topk_emulate(lg: torch.Tensor, k: int, mut=None):
    """The kernel in fp32: exp(l - max), k passes of a strict-greater scan, renormalise."""
    lf = lg.float()
    p = torch.exp(lf - lf.max(1, keepdim=True).values)
    den = p.sum(1, keepdim=True)
    E = lf.shape[1]
    ps = p[:, :E - 1] if mut == "last_expert_ignored" and E > k else p
    if mut == "tie_highest":
        ids = ps.shape[1] - 1 - torch.sort(ps.flip(1), dim=1, descending=True, stable=True).indices[:, :k]
    else:
        ids = torch.sort(ps, dim=1, descending=True, stable=True).indices[:, :k]
    w = p.gather(1, ids) / den
    if mut != "no_renorm":
        w = w / w.sum(1, keepdim=True)
    if mut == "weights_swapped":
        w = w.roll(1, 1)
    return w, ids.int()


def topk_mutation_applies(mut: str, T: int, E: int, k: int) -> bool:
    if mut == "weights_swapped":
        return k >= 2
    if mut == "no_renorm":
        return k < E
    if mut == "last_expert_ignored":                      # row 0 at k = 1 is all equal: expert 0 wins
        return k < E and (k >= 2 or T >= 4)
    return True


def assert_topk(w, ids, want_w, want_ids, what: str) -> None:
    w, ids = w.cpu().double(), ids.cpu().int()
    for j in range(ids.shape[1]):
        assert_equal(ids[:, j], want_ids[:, j], f"{what}: ids column {j}")
    err = (w - want_w).abs()
    assert bool((err <= 1e-5).all()), f"{what}: weight error {float(err.max())} in row {int(err.max(1).values.argmax())}"


# ====================================================================================================
# MoE align / sort / combine with hand-made routing
# ====================================================================================================
# R -> (T, k, per-expert row counts): an empty expert, an expert with all rows, counts 1, 64, 65, 256, 257, 513
MOE_ROUTINGS = {
    1: (1, 1, (0, 0, 1, 0)),
    255: (255, 1, (0, 255, 0, 0)),
    256: (128, 2, (64, 65, 0, 127)),
    257: (257, 1, (0, 0, 0, 257)),
    1026: (513, 2, (0, 1, 64, 65, 256, 513, 127, 0)),
}
MOE_MUTATIONS = ("row_dropped", "row_twice", "chunk_start_tail", "stale_table", "skip_last_j", "nonlocal_included",
                 "slice_drop", "slice_double")
MOE_COMBINE_SPLITS = (2, 4, 5, 8, 16)


def moe_windows(E: int, counts):
    """(e0, el): all experts, a window that excludes some, and one that holds no row."""
    empty = [e for e, c in enumerate(counts) if c == 0]
    return [(0, E), (1, E - 2), (empty[-1], 1)]


@functools.lru_cache(maxsize=8)
def moe_routing(R: int) -> torch.Tensor:
    """topk_ids int32 [T, k] written by hand: the flat rows are a fixed shuffle of the counts above."""
    T, k, counts = MOE_ROUTINGS[R]
    flat = torch.cat([torch.full((c,), e) for e, c in enumerate(counts)])
    perm = torch.randperm(R, generator=_gen(case_seed(R)))
    return flat[perm].int().view(T, k)


def moe_lists_want(ids: torch.Tensor, e0: int, el: int):
    """(counts [el], [sorted rows of expert e0 + e])"""
    flat = ids.flatten().long()
    rows = [(flat == e0 + e).nonzero().squeeze(1) for e in range(el)]
    return torch.tensor([len(r) for r in rows], dtype=torch.int32), rows


def moe_align_emulate(ids: torch.Tensor, e0: int, el: int, mut=None):
    """(counts int32 [el], lists int32 [el, R]); unwritten list entries hold -1."""
    R = ids.numel()
    counts, rows = moe_lists_want(ids, e0, el)
    rows = [r.flip(0) for r in rows]                      # any order within a list is legal
    big = int(counts.argmax())
    if mut == "row_dropped" and counts[big] > 0:
        rows[big] = rows[big][:-1]
    if mut == "row_twice" and counts[big] > 0 and el > 1:
        o = (big + 1) % el
        rows[o] = torch.cat([rows[o], rows[big][:1]])
    lists = torch.full((el, R), -1, dtype=torch.int32)
    for e, r in enumerate(rows):
        lists[e, :len(r)] = r.int()
    return torch.tensor([len(r) for r in rows], dtype=torch.int32), lists


def assert_align(counts, lists, ids, e0: int, el: int, what: str) -> None:
    wc, wr = moe_lists_want(ids, e0, el)
    counts, lists = counts.cpu(), lists.cpu()
    assert_equal(counts, wc, f"{what}: counts")
    for e in range(el):
        got = lists[e, :int(wc[e])].long().sort().values
        assert torch.equal(got, wr[e]), f"{what}: list of expert {e0 + e}"


def moe_sort_lists(ids: torch.Tensor, e0: int, el: int):
    """Hand-written counts and lists for ka_moe_sort: expert e's rows in descending order."""
    return moe_align_emulate(ids, e0, el)


def moe_sort_want(x: torch.Tensor, counts, lists, src_div: int, max_chunks: int, mut=None):
    """(xs [R, H] with SENT in unwritten rows, slot int32 [R] with -1 unwritten, tab int32 [max_chunks, 4];
    a stale table holds -1)."""
    R, H = lists.shape[1], x.shape[1]
    xs = torch.full((R, H), SENT, dtype=x.dtype)
    slot = torch.full((R,), -1, dtype=torch.int32)
    tab = torch.full((max_chunks, 4), -1 if mut == "stale_table" else 0, dtype=torch.int32)
    start = ch = 0
    for e, c in enumerate(counts.tolist()):
        slot[start:start + c] = lists[e, :c]
        xs[start:start + c] = x[(lists[e, :c] // src_div).long()]
        for j in range((c + 255) // 256):
            first = 256 * ch if mut == "chunk_start_tail" else start + 256 * j   # forgets the ragged tails before
            tab[ch] = torch.tensor([e, first, min(256, c - 256 * j), 0])
            ch += 1
        start += c
    return xs, slot, tab


def assert_sort(xs, slot, tab, want, what: str) -> None:
    wxs, wslot, wtab = want
    assert_equal(slot.cpu(), wslot, f"{what}: slot")
    assert_equal(tab.cpu().view(-1, 4), wtab, f"{what}: chunk table")
    assert_equal(xs.cpu(), wxs, f"{what}: xs")


def moe_combine_inputs(T: int, k: int, H: int, E: int = 8, split: int = 0):
    """(Y bf16 [T k, H] integers in [-5, 5] or P fp32 [split, T k, H], w fp32 [T, k] in {1/4, 1/2, 1}, ids)."""
    g = _gen(case_seed(T, k, H, split))
    Y = torch.randint(-4, 5, (T * k, H), generator=g).float()
    w = 2.0 ** torch.randint(-2, 1, (T, k), generator=g).float()
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).int()
    P = None
    if split:
        P, Y = int_slices(Y, split, case_seed(T, k, H, split, 1))
        assert float(Y.abs().max()) <= 5
    return Y.to(BF), P, w, ids


def moe_combine_want(Y, P, w, ids, e0: int, el: int, mut=None) -> torch.Tensor:
    """fp64 (exact) [T, H]; rows of non-local slots contribute nothing."""
    T, k = ids.shape
    y = (sum_slices(P, mut) if P is not None else Y.float()).double().view(T, k, -1)
    loc = (ids >= e0) & (ids < e0 + el)
    if mut == "nonlocal_included":
        loc = torch.ones_like(loc)
    if mut == "skip_last_j":
        loc = loc.clone()
        loc[:, k - 1] = False
    return (y * (w.double() * loc)[:, :, None]).sum(1)


def moe_poison_nonlocal(Y: torch.Tensor, ids, e0: int, el: int) -> torch.Tensor:
    """Y (or P) with the rows of non-local slots set to 99: the combine must not read them into the sum."""
    loc = ((ids >= e0) & (ids < e0 + el)).flatten()
    Y = Y.clone()
    Y[..., ~loc, :] = 99.0
    return Y


def moe_dense_ref(x, w13, w2, tw, tid, e0):
    """fp32 reference of the local experts' weighted FFN (activation rounded to bf16 like the kernels)."""
    T, H = x.shape
    el, two_i, _ = w13.shape
    I = two_i // 2
    out = torch.zeros(T, H, device=x.device)
    for e in range(el):
        sel = (tid.long() == e0 + e)
        wt = (tw * sel).sum(1)
        rows = torch.nonzero(sel.any(1)).squeeze(1)
        if rows.numel() == 0:
            continue
        g = x[rows].float() @ w13[e].float().t()
        a = (torch.nn.functional.silu(g[:, :I]) * g[:, I:]).to(BF).float()
        out[rows] += wt[rows].unsqueeze(1) * (a @ w2[e].float().t())
    return out
