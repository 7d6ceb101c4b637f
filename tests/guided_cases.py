"""Shared cases of the guided-decoding mask (ops.guide_mask, csrc/guide_mask.hip) and a literal pure-Python
reference of it: a loop over rows, tokens and bytes that shares no code with ops/reference.py or the kernel.

Vocabularies are synthetic: `None` entries (every id with id % 7 == 3, and the two EOS ids, V - 1 and 5, so the
fallback bit of an empty row is the last valid bit of the row), byte strings of 1, 2, 15, 16, 17 and 40 bytes
that are live under the guides and copies of them whose last byte is wrong (the last byte of the 16-byte
record, the first and the last of the overflow pool), and, from V = 520 up, all 256 single bytes (a smaller
vocabulary cannot hold them: it gets the strings the guides use first).

Every case holds guide A (`a(bc)+[d;]?`), guide B (choices pods / nodes / po) and an unused guide C between
them at different arena bases; the arena around them is filled with values that look like live states, so a
lookup outside a guide's range shows.  Rows cycle through: not guided; each guide in its start state, a mid
state, an accepting state with outgoing edges and one with none; every pending mode; base rows -1, FIRST and
BODY of a real `build_masks` (FIRST admits only tokens that start with a space, which neither guide does: those
rows' intersections are empty by construction and fall back to EOS).
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ai_agent_kubectl_amd.engine import guided
from ai_agent_kubectl_amd.engine.safe_decode import MASK_BODY, MASK_FIRST, build_masks

TILE = 1024   # tokens per workgroup: ka_guide_mask_tile(), asserted by the GPU test
ARENA = 96    # states of the cases' arena

LIVE = [b"a", b"bc", b"d", b";", b"abc", b"bcbc", b"abcd", b"bcd", b"bc;", b"p", b"po", b"pod", b"pods", b"ds", b"s",
        b"nodes", b"no", b"des", b"o", b"n",
        b"a" + b"bc" * 7, b"bc" * 8, b"a" + b"bc" * 8, b"bc" * 20,                    # 15, 16, 17, 40 bytes, live
        b"a" + b"bc" * 6 + b"bx", b"bc" * 7 + b"bx", b"a" + b"bc" * 7 + b"bx", b"bc" * 19 + b"bx",   # ... the last byte dead
        b"xc" + b"bc" * 7, b"ac" + b"bc" * 19,                                          # the first / second byte dead
        b" a", b" po", b" bc", b"0", b"12", b"ab", b"b", b"c", b"x"]
LENGTHS = {1, 2, 15, 16, 17, 40}


class Tok:
    """What build_masks reads of a tokenizer."""

    def __init__(self, vocab, eos_ids):
        self.id_to_bytes, self.eos_ids, self.vocab_size = vocab, eos_ids, len(vocab)


@functools.lru_cache(maxsize=None)
def vocabulary(V: int):
    rng = random.Random(V)
    singles = [bytes([b]) for b in range(256)]
    rng.shuffle(singles)
    items = LIVE + [s for s in singles if s not in LIVE]
    eos_ids = (V - 1, 5)
    vocab: List[Optional[bytes]] = [None] * V
    k = 0
    for i in range(V):
        if i % 7 == 3 or i in eos_ids:
            continue
        if k < len(items):
            vocab[i] = items[k]
        else:
            vocab[i] = rng.choice(LIVE) + (rng.choice(LIVE) if rng.random() < 0.5 else b"")
        k += 1
    return vocab, eos_ids


@functools.lru_cache(maxsize=None)
def guides():
    a = guided.compile_regex(r"a(bc)+[d;]?")
    b = guided.compile_choice(["pods", "nodes", "po"])
    c = guided.compile_regex(r"\d+")
    return a, b, c


@functools.lru_cache(maxsize=None)
def arena():
    """-> (trans uint16 [ARENA, 256], accept uint8 [ARENA], base of A, base of B)."""
    a, b, c = guides()
    rng = np.random.RandomState(7)
    trans = rng.randint(0, 4, size=(ARENA, 256)).astype(np.uint16)   # live-looking filler
    accept = np.ones(ARENA, dtype=np.uint8)
    base_a = 3
    base_c = base_a + a.nstates + 1
    base_b = base_c + c.nstates + 2
    assert base_b + b.nstates < ARENA
    for g, base in ((a, base_a), (c, base_c), (b, base_b)):
        trans[base:base + g.nstates] = g.trans
        accept[base:base + g.nstates] = g.accept
    return trans, accept, base_a, base_b


# state kinds: (guide index, bytes that lead there from the start)
STATES = [(0, b""), (0, b"a"), (0, b"abc"), (0, b"abcd"), (1, b""), (1, b"p"), (1, b"po"), (1, b"pods")]
PENDS = ["none", "live", "kill", "eos", "past_v", "negative", "byteless", "other_row", "past_n"]
BASES = [-1, MASK_BODY, MASK_BODY, -1, MASK_FIRST]


@dataclass
class Case:
    V: int
    rows: int
    vocab: list
    eos_ids: tuple
    trans: np.ndarray
    accept: np.ndarray
    row_base: np.ndarray
    row_nstates: np.ndarray
    row_state: np.ndarray
    pend_src: Optional[np.ndarray]
    tokens: Optional[np.ndarray]
    base_bits: Optional[np.ndarray]
    base_idx: Optional[np.ndarray]
    kinds: list     # per row: None, or (state kind, pending mode)
    _literal: Optional[tuple] = None

    @property
    def id(self) -> str:
        first = next(k for k in self.kinds if k)
        return f"V{self.V}-R{self.rows}-{'base' if self.base_bits is not None else 'nobase'}" \
               f"-{'pend' if self.pend_src is not None else 'nopend'}-s{first[0]}{first[1]}"


def _first(vocab, pred):
    return next(i for i, p in enumerate(vocab) if p and pred(p))


def make_case(V: int, rows: int, with_base: bool, with_pend: bool = True, shift: int = 0) -> Case:
    vocab, eos_ids = vocabulary(V)
    trans, accept, base_a, base_b = arena()
    gs = guides()
    n_tok = rows + 2
    row_base = np.full(rows, -1, dtype=np.int32)
    row_n = np.zeros(rows, dtype=np.int32)
    row_state = np.zeros(rows, dtype=np.int32)
    pend = np.full(rows, -1, dtype=np.int32)
    tokens = np.zeros(n_tok, dtype=np.int32)
    base_idx = np.full(rows, -1, dtype=np.int32)
    kinds: list = [None] * rows
    k = shift
    for r in range(rows):
        # rows 0, 3, 6, ... are not guided (a single row is guided); their base rows still vary
        base_idx[r] = BASES[(r + shift) % len(BASES)]
        if rows > 1 and r % 3 == 0:
            tokens[r] = (r * 37) % V
            continue
        gi, lead = STATES[k % len(STATES)]
        mode = PENDS[k % len(PENDS)]
        k += 1
        g = gs[gi]
        s = g.walk(0, lead)
        assert s >= 0
        row_base[r] = (base_a, base_b)[gi]
        row_n[r] = g.nstates
        row_state[r] = s
        pend[r] = r
        if mode == "none":
            pend[r] = -1
        elif mode == "live":
            try:
                tokens[r] = _first(vocab, lambda p: g.walk(s, p) >= 0)
            except StopIteration:   # an accepting state without edges: every token kills
                tokens[r] = _first(vocab, lambda p: True)
        elif mode == "kill":
            tokens[r] = _first(vocab, lambda p: g.walk(s, p) < 0)
        elif mode == "eos":
            tokens[r] = eos_ids[r % 2]
        elif mode == "past_v":
            tokens[r] = V + r
        elif mode == "negative":
            tokens[r] = -1 - r
        elif mode == "byteless":
            tokens[r] = 3      # 3 % 7 == 3: None, and not an EOS id
        elif mode == "other_row":
            pend[r] = (r + 1) % n_tok if rows > 1 else rows
        elif mode == "past_n":
            pend[r] = n_tok + r
        kinds[r] = (k - 1) % len(STATES), mode
    tokens[rows] = _first(vocab, lambda p: p in (b"a", b"p"))
    tokens[rows + 1] = V - 1
    bits = build_masks(Tok(vocab, eos_ids)) if with_base else None
    return Case(V, rows, vocab, eos_ids, trans, accept, row_base, row_n, row_state, pend if with_pend else None,
                tokens if with_pend else None, bits, base_idx if with_base else None, kinds)


def _cases():
    out = []
    shift = 0
    for V in (33, 64, 65, 520, TILE - 1, TILE, TILE + 1, 128256):
        for rows in (1, 3, 64):
            if rows == 64 and V > TILE + 1:
                continue   # the literal reference stays within seconds
            if rows < 64:   # shift 0: a row in its start state with nothing pending, a mask with many bits
                out.append(make_case(V, rows, with_base=rows != 1, shift=0))
            out.append(make_case(V, rows, with_base=rows != 1, shift=shift + 1))
            shift += 5
    # the single-row cases again with a base table, so FIRST / BODY also meet every V alone; no base table
    # and no pending arrays at all beside several rows
    out += [make_case(V, 1, True, shift=V) for V in (33, 65, TILE + 1)]
    out += [make_case(520, 3, False, shift=1), make_case(65, 3, True, with_pend=False, shift=2),
            make_case(TILE + 1, 64, False, with_pend=False, shift=3)]
    return out


CASES = _cases()


def check_preconditions():
    """What the cases promise (module docstring), asserted on the cases themselves."""
    a, b, c = guides()
    trans, accept, base_a, base_b = arena()
    assert len({base_a, base_b}) == 2 and base_a + a.nstates < base_b - c.nstates
    assert {len(p) for p in LIVE} >= LENGTHS
    assert {c.V for c in CASES} == {33, 64, 65, 520, TILE - 1, TILE, TILE + 1, 128256}
    assert {c.rows for c in CASES} == {1, 3, 64}
    for V in {c.V for c in CASES}:
        vocab, eos = vocabulary(V)
        assert len(eos) == 2 and all(vocab[e] is None for e in eos) and vocab[3] is None
        if V >= 520:
            assert {bytes([x]) for x in range(256)} <= {p for p in vocab if p}
            assert {len(p) for p in vocab if p} >= LENGTHS
    # the four state kinds of both guides
    for gi, g in enumerate((a, b)):
        leads = [lead for i, lead in STATES if i == gi]
        st = [g.walk(0, lead) for lead in leads]
        out = [(g.trans[s] != guided.DEAD).any() for s in st]
        acc = [bool(g.accept[s]) for s in st]
        assert st[0] == 0 and not acc[0] and not acc[1] and out[1]
        assert acc[2] and out[2] and acc[3] and not out[3]
    seen_states, seen_pend, seen_base = set(), set(), set()
    for c in CASES:
        for r, kind in enumerate(c.kinds):
            if kind is None:
                assert c.row_base[r] < 0
                continue
            assert 0 <= c.row_state[r] < c.row_nstates[r] and c.row_base[r] + c.row_nstates[r] <= ARENA
            seen_states.add(kind[0])
            if c.pend_src is not None:
                seen_pend.add(kind[1])
            seen_base.add("none" if c.base_idx is None else int(c.base_idx[r]))
        if c.rows == 64:   # guided rows between rows that are not, both guides, every state kind
            assert c.row_base[0] < 0 and c.row_base[63] < 0 and {base_a, base_b} <= set(c.row_base.tolist())
            assert {k[0] for k in c.kinds if k} == set(range(len(STATES)))
    assert seen_states == set(range(len(STATES))) and seen_pend == set(PENDS)
    assert seen_base == {"none", -1, MASK_FIRST, MASK_BODY}
    # a row whose intersection with its base row is empty by construction: FIRST under either guide
    empties = 0
    for c in CASES[:12]:
        bits, idx, after = literal(c)
        n_static = 0 if c.base_bits is None else c.base_bits.shape[0]
        for r, kind in enumerate(c.kinds):
            if kind and c.base_idx is not None and c.base_idx[r] == MASK_FIRST and after[r] >= 0:
                row = bits[n_static + r]
                e0 = c.eos_ids[0]
                assert int(row.sum()) == int(row[e0 >> 5]) == 1 << (e0 & 31)
                empties += 1
    assert empties > 0
    # every vocabulary size meets a mask with many bits, the large ones over several words / workgroup tiles
    for V in {c.V for c in CASES}:
        best = np.zeros(1, dtype=np.uint32)
        for c in CASES:
            if c.V == V:
                bits = literal(c)[0][0 if c.base_bits is None else c.base_bits.shape[0]:]
                row = max(bits, key=lambda b: int(np.count_nonzero(b)))
                best = row if np.count_nonzero(row) > np.count_nonzero(best) else best
        assert np.unpackbits(best.view(np.uint8)).sum() >= 4
        if V >= TILE - 1:
            assert np.count_nonzero(best) >= 8
        if V > 2 * TILE:
            assert len(set(np.flatnonzero(best) // (TILE // 32))) > 50


def literal_uncached(c: Case):
    """-> (bits uint32 [n_static + rows, words], idx int32 [rows], state_after int32 [rows])."""
    V, R = c.V, c.rows
    words = (V + 31) // 32
    n_static = 0 if c.base_bits is None else int(c.base_bits.shape[0])
    bits = [[0] * words for _ in range(n_static + R)]
    for i in range(n_static):
        bits[i] = [int(x) for x in c.base_bits[i]]
    idx, after = [-1] * R, [-1] * R
    table = c.trans.tolist()
    n_tokens = 0 if c.tokens is None else len(c.tokens)
    for r in range(R):
        b0 = int(c.row_base[r])
        if b0 < 0:
            idx[r] = int(c.base_idx[r]) if c.base_idx is not None else -1
            continue
        idx[r] = n_static + r
        n = int(c.row_nstates[r])
        s = int(c.row_state[r])

        def nxt(state: int, byte: int) -> int:
            v = table[b0 + state][byte]
            return v if v < n else -1

        ps = int(c.pend_src[r]) if c.pend_src is not None else -1
        if 0 <= ps < n_tokens:
            t = int(c.tokens[ps])
            if t in c.eos_ids:
                pass
            elif t < 0 or t >= V or not c.vocab[t]:
                s = -1
            else:
                for byte in c.vocab[t]:
                    if s >= 0:
                        s = nxt(s, byte)
        after[r] = s
        base_row = None
        if c.base_bits is not None and c.base_idx[r] >= 0:
            base_row = bits[int(c.base_idx[r])]
        count = 0
        for t in range(V):
            ok = t in c.eos_ids and s >= 0 and bool(c.accept[b0 + s])
            data = c.vocab[t]
            if not ok and data and s >= 0:
                cur = s
                for byte in data:
                    cur = nxt(cur, byte)
                    if cur < 0:
                        break
                ok = cur >= 0
            if ok and base_row is not None:
                ok = bool((base_row[t >> 5] >> (t & 31)) & 1)
            if ok:
                bits[n_static + r][t >> 5] |= 1 << (t & 31)
                count += 1
        if count == 0:
            e0 = c.eos_ids[0]
            bits[n_static + r][e0 >> 5] |= 1 << (e0 & 31)
    return (np.asarray(bits, dtype=np.uint32).reshape(n_static + R, words), np.asarray(idx, dtype=np.int32),
            np.asarray(after, dtype=np.int32))


def literal(c: Case):
    """The literal reference, computed once per case and shared (read-only arrays)."""
    if c._literal is None:
        c._literal = literal_uncached(c)
        for a in c._literal:
            a.setflags(write=False)
    return c._literal


@functools.lru_cache(maxsize=None)
def token_table(V: int, device: str = "cpu"):
    from ai_agent_kubectl_amd import ops
    vocab, eos_ids = vocabulary(V)
    return ops.token_table(vocab, eos_ids, device)


def run_ops(c: Case, device: str = "cpu"):
    """ops.guide_mask on the case -> the three tensors."""
    import torch
    from ai_agent_kubectl_amd import ops

    def dev(a, view=None):
        if a is None:
            return None
        return torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view))).to(device)

    return ops.guide_mask(token_table(c.V, device), dev(c.trans, np.int16), dev(c.accept), dev(c.row_base),
                          dev(c.row_nstates), dev(c.row_state), dev(c.pend_src), dev(c.tokens),
                          dev(c.base_bits, np.int32), dev(c.base_idx))


def chain_async(eng, seq):
    """Run `seq` through launch_prefill_async and chained launch_decode_async steps, each decode step queued
    while the previous token is still on the device, until the sequence finishes (EOS or max_new_tokens); the
    step queued behind the one that finished it is read back and discarded, as the engine does."""
    from ai_agent_kubectl_amd.engine.scheduler import Batch
    sch = eng.scheduler
    sch.add(seq)
    gather, sch.gather_max_s = sch.gather_max_s, 0.0   # everything is here
    try:
        batch = sch.schedule()
    finally:
        sch.gather_max_s = gather
    assert batch.seqs == [seq]
    h = eng.runner.launch_prefill_async(batch)
    while True:
        nxt = nh = None
        if seq.num_generated + 1 < seq.params.max_new_tokens:
            eng.bm.ensure_capacity(seq.block_table, seq.total_len + 1)
            nxt = Batch([seq], [1], is_decode=True)
            nh = eng.runner.launch_decode_async(nxt, chained=True)
        eng._apply(batch, eng.runner.collect(h))
        sch.on_step_done(batch)
        if seq.finished:
            if nh is not None:
                eng.runner.collect(nh)
            return seq.output_ids
        batch, h = nxt, nh
