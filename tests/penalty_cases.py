"""Cases of tests/test_penalties_gpu.py / test_penalties_cpu.py and a numpy-float32 reference of
ops.logit_adjust that follows the issue's formula literally, one rounded fp32 operation per line:

    x = float(bf16 logit)
    if seen and r != 1:  x = (x > 0) ? x / r : x * r
    x = x - (frequency * float(c))
    x = x - (c > 0 ? presence : 0)
    x = x + bias
    logit = bf16 round-to-nearest-even(x)

It shares no code with ops/reference.py (torch) or the kernel: bf16 is handled as uint16 bit patterns.
Comparisons are exact (`==` on the patterns of the whole [R, V] tensor), so there is no tolerance to derive.

Geometry.  V, R, offsets: the sampler's set.  Entries per row rotate through COUNTS: 0, 1, the workgroup
size -1 / +0 / +1 (a thread with and without an entry in the first round), one full batch per thread
-1 / +0 / +1 (the second round of the kernel's loop starts there) and 9000 (the prompt set of a long
request: several rounds), capped at V.  A row's ids are distinct and include 0 and V - 1 of the slice, a
run of 512 consecutive ids in entry order (neighbouring tokens of one dword owned by different threads)
and, from four entries up, ids outside [off, off + V) on both sides, which must be skipped.  Every fourth
row is a neutral one with an empty segment.  Every case asserts these preconditions itself.
"""
import functools

import numpy as np
import torch

NT = 256            # csrc/logit_adjust.hip LA_NT (test_penalties_gpu asserts both against the library)
BATCH = 2048        # LA_NT * LA_UN
PROMPT_BIT = 0x80000000

VOCABS = (8, 520, 32776, 128256)
ROWS = (1, 3, 64)
OFFSETS = (0, 64)
CASES = [(V, R, off) for V in VOCABS for R in ROWS for off in OFFSETS]

COUNTS = (0, 1, NT - 1, NT, NT + 1, BATCH - 1, BATCH, BATCH + 1, 9000)
# (presence, frequency, repetition)
PARAMS = ((0.0, 0.0, 1.0),        # logit_bias alone
          (1.5, 0.0, 1.0),
          (0.0, 0.75, 1.0),
          (0.0, 0.0, 1.3),
          (-2.0, 2.0, 0.5),
          (0.3, -1.1, 2.0),
          (0.0625, 0.001, 1.0))   # adjustments around half a bf16 ulp
PENDS = ("none", "first", "last", "middle", "new", "outside", "other_row")
CNTS = np.array([0, 0, 1, 1, 2, 7, 1000, (1 << 31) - 2], dtype=np.uint32)   # + 1 for a pending token still fits
BIASES = np.array([0.0, 0.0, 0.0, 100.0, -100.0, 0.001, -3.25, 17.5], dtype=np.float32)


def case_id(case) -> str:
    return "V{}-R{}-off{}".format(*case)


# ---------------- bf16 as bit patterns ----------------
def bf16_to_f32(u16: np.ndarray) -> np.ndarray:
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x: np.ndarray) -> np.ndarray:
    """Round to nearest, ties to even; NaN stays NaN (quiet), infinities stay."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def adjust_values(raw_u16, c, prompt, bias, presence, frequency, repetition) -> np.ndarray:
    """The formula for arrays of entries of one row -> bf16 patterns.  Every line is one fp32 operation."""
    f = np.float32
    pres, freq, rep = f(presence), f(frequency), f(repetition)
    x = bf16_to_f32(np.asarray(raw_u16, dtype=np.uint16))
    c = np.asarray(c, dtype=np.int64)
    seen = np.asarray(prompt, dtype=bool) | (c > 0)
    with np.errstate(all="ignore"):
        if rep != f(1.0):
            x = np.where(seen, np.where(x > f(0.0), (x / rep).astype(f), (x * rep).astype(f)), x).astype(f)
        prod = (freq * c.astype(f)).astype(f)
        x = (x - prod).astype(f)
        x = (x - np.where(c > 0, pres, f(0.0)).astype(f)).astype(f)
        x = (x + np.asarray(bias, dtype=f)).astype(f)
    return f32_to_bf16(x)


def np_reference(logits_u16, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src, tokens,
                 off: int):
    """-> (adjusted patterns [R, V], saved patterns [R + E], slots written bool [R + E])."""
    out = logits_u16.copy()
    R, V = out.shape
    E = len(ent_id)
    saved = np.zeros(R + E, dtype=np.uint16)
    written = np.zeros(R + E, dtype=bool)
    for r in range(R):
        e0, e1 = int(row_start[r]), int(row_start[r + 1])
        ps = int(pend_src[r]) if pend_src is not None else -1
        pend = int(tokens[ps]) if 0 <= ps < len(tokens) else -1
        neutral = presence[r] == 0 and frequency[r] == 0 and repetition[r] == 1
        if e0 == e1 and (pend < 0 or neutral):
            continue
        ids = ent_id[e0:e1].astype(np.int64)
        word = ent_cnt[e0:e1].astype(np.int64) & 0xFFFFFFFF
        c = word & (PROMPT_BIT - 1)
        prompt = (word & PROMPT_BIT) != 0
        bias = ent_bias[e0:e1].astype(np.float32)
        slot = np.arange(e0, e1) + R
        if pend >= 0:
            hit = ids == pend
            assert hit.sum() <= 1
            if hit.any():
                c = c + hit
            else:
                ids, c, prompt = np.append(ids, pend), np.append(c, 1), np.append(prompt, False)
                bias, slot = np.append(bias, np.float32(0.0)), np.append(slot, r)
        li = ids - off
        ok = (li >= 0) & (li < V)
        li = li[ok]
        raw = out[r, li]
        saved[slot[ok]] = raw
        written[slot[ok]] = True
        out[r, li] = adjust_values(raw, c[ok], prompt[ok], bias[ok], presence[r], frequency[r], repetition[r])
    return out, saved, written


# ---------------- case builders ----------------
def make_logits(R: int, V: int, seed: int) -> np.ndarray:
    """bf16 patterns: randn * 4 with a few zeros, -0, infinities and large values."""
    g = torch.Generator().manual_seed(seed)
    l = (torch.randn(R, V, generator=g) * 4).to(torch.bfloat16)
    u = l.view(torch.int16).numpy().view(np.uint16).copy()
    rs = np.random.RandomState(seed)
    for pat in (0x0000, 0x8000, 0xFF80, 0x7F80, 0x4780, 0xC780, 0x0001):   # 0, -0, -inf, +inf, 65536, -65536, a subnormal
        u[rs.randint(0, R, size=max(1, R * V // 64)), rs.randint(0, V, size=max(1, R * V // 64))] = pat
    return u


def row_ids(rs, n: int, V: int, off: int) -> np.ndarray:
    """n distinct global ids: 0 and V - 1 of the slice, a run of 512 consecutive ids (n >= 600), ids outside
    the slice on both sides (n >= 4), the rest random."""
    n = min(n, V)
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    outside = ([off + V + 5] + ([3] if off > 0 else [])) if n >= 4 else []
    fixed = {0} if n - len(outside) == 1 else {0, V - 1}
    run = np.zeros(0, dtype=np.int64)
    if n >= 600:
        s = int(rs.randint(1, V - 513)) | 1     # an odd start: the run's dwords straddle thread pairs both ways
        run = np.arange(s, s + 512)
    taken = fixed | set(run.tolist())
    need = n - len(outside) - len(taken)
    pool = np.setdiff1d(np.arange(V), np.fromiter(taken, dtype=np.int64), assume_unique=False)
    rest = rs.choice(pool, size=need, replace=False) if need > 0 else np.zeros(0, dtype=np.int64)
    loose = np.concatenate([np.fromiter(fixed, dtype=np.int64), rest]) + off
    loose = np.concatenate([loose, np.asarray(outside, dtype=np.int64)])
    rs.shuffle(loose)
    k = int(rs.randint(0, len(loose) + 1))
    return np.concatenate([loose[:k], run + off, loose[k:]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def build(case):
    """Inputs (numpy) and the numpy reference of one case, computed once and shared."""
    V, R, off = case
    no = CASES.index(case) if case in CASES else 97
    rs = np.random.RandomState(4000 + no)
    logits = make_logits(R, V, 4000 + no)
    row_start = np.zeros(R + 1, dtype=np.int32)
    presence, frequency = np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.float32)
    repetition = np.ones(R, dtype=np.float32)
    pend_src = np.full(R, -1, dtype=np.int32)
    tokens = rs.randint(off, off + V, size=R + 3).astype(np.int32)   # more slots than rows, like d_out
    ids_l, modes = [], []
    a = no   # counts the active rows, shifted per case so that one-row cases differ
    for r in range(R):
        if R > 1 and r % 4 == 3:   # a neutral row between active ones
            ids_l.append(np.zeros(0, dtype=np.int32))
            modes.append(("neutral", 0))
        else:
            ids = row_ids(rs, COUNTS[a % len(COUNTS)], V, off)
            presence[r], frequency[r], repetition[r] = PARAMS[a % len(PARAMS)]
            mode = PENDS[a % len(PENDS)]
            n = len(ids)
            inside = np.nonzero((ids >= off) & (ids < off + V))[0]
            if mode in ("first", "last", "middle") and len(inside) == 0:
                mode = "new"
            if mode != "none":
                slot = (r + 1) % (R + 3) if mode == "other_row" else r   # another row's d_out slot
                pend_src[r] = slot
                if mode in ("first", "last", "middle"):
                    tokens[slot] = ids[inside[{"first": 0, "last": -1, "middle": len(inside) // 2}[mode]]]
                elif mode == "outside":
                    tokens[slot] = off + V + 9
                elif mode == "other_row":
                    pass   # whatever that slot holds, or will hold once its own row has been built
                else:   # an id no entry of the row has
                    free = np.setdiff1d(np.arange(off, off + V), ids)
                    if len(free):
                        tokens[slot] = free[rs.randint(len(free))]
                    else:
                        mode, tokens[slot] = "first", ids[inside[0]]
            ids_l.append(ids)
            modes.append((mode, n))
            a += 1
        row_start[r + 1] = row_start[r] + len(ids_l[-1])
    # a slot written for a later row may not change an earlier row's choice: check_preconditions re-derives it
    ent_id = np.concatenate(ids_l).astype(np.int32) if ids_l else np.zeros(0, dtype=np.int32)
    E = len(ent_id)
    ent_cnt = (CNTS[rs.randint(0, len(CNTS), size=E)] | (rs.randint(0, 2, size=E).astype(np.uint32) << np.uint32(31)))
    ent_bias = BIASES[rs.randint(0, len(BIASES), size=E)]
    inp = dict(logits=logits, row_start=row_start, ent_id=ent_id, ent_cnt=ent_cnt.astype(np.uint32).view(np.int32),
               ent_bias=ent_bias.astype(np.float32), presence=presence, frequency=frequency, repetition=repetition,
               pend_src=pend_src, tokens=tokens, off=off, modes=modes)
    check_preconditions(inp)
    out, saved, written = np_reference(logits, row_start, ent_id, inp["ent_cnt"], ent_bias, presence, frequency,
                                       repetition, pend_src, tokens, off)
    return inp, dict(logits=out, saved=saved, written=written)


def check_preconditions(inp) -> None:
    """Distinct ids per row, ids in range, segment lengths, and each row's pending mode still what was built."""
    R, V = inp["logits"].shape
    off, rs_, ids, tok = inp["off"], inp["row_start"], inp["ent_id"], inp["tokens"]
    assert rs_[0] == 0 and rs_[-1] == len(ids) == len(inp["ent_cnt"]) == len(inp["ent_bias"])
    assert bool((np.diff(rs_) >= 0).all()) and len(tok) == R + 3
    assert bool((ids >= 0).all()) and bool((ids < off + V + 64).all())
    for r, (mode, n) in enumerate(inp["modes"]):
        seg = ids[rs_[r]:rs_[r + 1]]
        assert len(seg) == n and len(np.unique(seg)) == n, (r, "ids repeat or a segment length is off")
        ps = int(inp["pend_src"][r])
        if mode == "neutral":
            assert n == 0 and ps == -1 and (inp["presence"][r], inp["frequency"][r], inp["repetition"][r]) == (0, 0, 1)
            continue
        if n >= 2:
            assert off in seg and off + V - 1 in seg
        if n >= 4:
            assert off + V + 5 in seg and (off == 0 or 3 in seg)
        if n >= 600:
            assert bool((np.diff(seg) == 1).sum() >= 511)
        inside = seg[(seg >= off) & (seg < off + V)]
        if mode == "none":
            assert ps == -1
            continue
        assert 0 <= ps < R + 3 and (ps != r) == (mode == "other_row")
        t = int(tok[ps])
        if mode == "other_row":
            continue
        if mode in ("first", "last", "middle"):
            assert t == int(inside[{"first": 0, "last": -1, "middle": len(inside) // 2}[mode]])
        elif mode == "outside":
            assert t >= off + V
        else:
            assert off <= t < off + V and t not in seg


def as_torch(inp, device="cpu"):
    """The case's arrays as the tensors ops.logit_adjust takes (logits bf16, a fresh copy)."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in inp.items() if isinstance(v, np.ndarray)}
    t["logits"] = torch.from_numpy(inp["logits"].view(np.int16).copy()).view(torch.bfloat16).to(device)
    return t


def bits(t: torch.Tensor) -> torch.Tensor:
    """bf16 tensor -> its int16 patterns on the CPU."""
    return t.detach().cpu().contiguous().view(torch.int16)


def want_bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16).copy())


# ---------------- the host packer's oracle ----------------
def counter_oracle(prompt_ids, output_ids, bias: dict, repetition: float, placeholder: int = -1):
    """{token id: (c, in the prompt, bias)} as the issue defines a row's entries, from collections.Counter:
    c over output_ids without a trailing placeholder; the entries are the tokens with c > 0, the bias ids
    and, when repetition != 1 (the only reader of the prompt bit), the prompt's ids."""
    from collections import Counter
    out = list(output_ids)
    if out and out[-1] == placeholder:
        out.pop()
    c = Counter(out)
    prompt = set(prompt_ids)
    keys = set(c) | set(bias) | (prompt if repetition != 1 else set())
    return {t: (c.get(t, 0), t in prompt, float(bias.get(t, 0.0))) for t in keys}


if __name__ == "__main__":
    import time
    t0 = time.time()
    for case in CASES:
        inp, want = build(case)
        changed = int((want["logits"] != inp["logits"]).sum())
        print(case_id(case), "entries", len(inp["ent_id"]), "changed", changed,
              "pend", sorted({m for m, _ in inp["modes"]}))
    print(f"{time.time() - t0:.1f} s")
