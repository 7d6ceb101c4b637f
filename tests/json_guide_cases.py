"""Shared cases of the stack-guide mask (ops.guide_mask_stack, csrc/guide_stack.hip: JSON mode) and a literal
pure-Python reference of it: a loop over rows, tokens and bytes that shares no code with ops/reference.py, the
kernel or StackGuide.walk.

Vocabularies are synthetic, as in guided_cases: `None` entries (every id with id % 7 == 3, and the two EOS ids,
V - 1 and 5), then LIVE: single structural bytes, tokens that cross the stack edges (`}}`, `]]`, `]}`, `[]`, `[]]`:
push one, pop two, from the token's own pushes into the row's stack; `{"a":[`, `":`, `,"`, `1}`, `e+`), 15 x `[`,
overflow tokens of 16, 17 and 40 bytes with 16 and 17 live pushes (one side of the per-token limit each), a 40-byte
token that pushes and pops in turn, copies of them with the last byte wrong, a token that ends inside a UTF-8
sequence and the one that completes it; from V = 520 up all 256 single bytes.

Every case holds the json_object guide J, a small schema guide S with a free-form position and regex guide A of
guided_cases at different arena bases; the arena and arena_pop around them are filled with values that look live.
Rows cycle through: not guided; a DFA-kind row (A); stack rows of J at depths 0, 1, 7, 8, 9 (the word boundary),
15, 16, 17, 63 and 64, inside a number, inside a UTF-8 sequence and in the final state; a closing token on an empty
stack; corrupt depths (65, -1) and a symbol 0 below the depth; rows of S; every pending mode of guided_cases plus
a pending token that pushes, one that pops to depth 0 and one that dies on the per-token limit; base rows -1,
FIRST and BODY.
"""
from __future__ import annotations

import functools
import math
import random
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ai_agent_kubectl_amd.engine import guided
from ai_agent_kubectl_amd.engine.safe_decode import MASK_BODY, MASK_FIRST, build_masks
from tests.guided_cases import Tok

TILE = 1024   # tokens per workgroup: ka_guide_mask_stack_tile(), asserted by the GPU test

P16, P17 = b"[" * 16, b"[" * 17
TURN = b"[]," * 13 + b"["     # 40 bytes: pushes and pops in turn, one symbol deeper at its end
STRUCT = [b"}}", b"]]", b"]}", b"[]", b"[]]", b'{"a":[', b'":', b',"', b"1}", b"e+", b"[" * 15,
          P16, P17, P16 + b"]" * 24, P17 + b"]" * 23, TURN]
UTF8_HEAD, UTF8_TAIL = b'"\xc3', b'\xa9"'
LIVE = [b"{", b"}", b'"', b":", b",", b"[", b"]", b"1", b"a", b" ", b"t", b"b", b"c"] + STRUCT \
    + [t[:-1] + b"\x00" for t in STRUCT] + [UTF8_HEAD, UTF8_TAIL, b"\xa9", b"abc", b"bc", b'{"k":1', b"-", b"0"]
SCHEMA = {"type": "object", "properties": {"a": {"type": "array", "items": {"type": "integer"}, "maxItems": 2},
                                           "x": {}}, "required": ["a"]}


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
    return guided.compile_json_object(), guided.compile_json_schema(SCHEMA), guided.compile_regex(r"a(bc)+[d;]?")


@functools.lru_cache(maxsize=None)
def arena():
    """-> (trans uint16 [G, 256], accept uint8 [G], pop uint16 [G, 16], bases of J, S, A)."""
    gs = guides()
    bases, at = [], 5
    for g in gs:
        bases.append(at)
        at += g.nstates + 3
    G = at + 4
    rng = np.random.RandomState(11)
    trans = rng.randint(0, 4, size=(G, 256)).astype(np.uint16)   # live-looking filler
    accept = np.ones(G, dtype=np.uint8)
    pop = rng.randint(0, 4, size=(G, 16)).astype(np.uint16)
    for g, base in zip(gs, bases):
        trans[base:base + g.nstates] = g.trans
        accept[base:base + g.nstates] = g.accept
        if isinstance(g, guided.StackGuide):
            pop[base] = g.pop_to
    return trans, accept, pop, tuple(bases)


J, S, A = 0, 1, 2
K = b'{"k":'
DEPTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64)
# state kinds: (guide, the bytes that lead there from the start, a corruption of the row or None)
STATES = [(J, b"", None)] + [(J, K + b"[" * (d - 1), None) for d in DEPTHS[1:]] + [
    (J, K + b"[[1", None), (J, K + UTF8_HEAD, None), (J, b"{}", None), (J, K + b"1", None), (J, K + b'["ab', None),
    (J, K + b"[1", "empty"), (J, K + b"[", "depth65"), (J, K + b"[", "depth-1"), (J, K + b"[[", "sym0"),
    (S, b"", None), (S, b'{"a":[1', None), (S, b'{"a":[],"x":[{"q":[', None), (S, b'{"a":[1,2]}', None),
    (A, b"", None), (A, b"abc", None)]
PENDS = ["none", "live", "kill", "eos", "past_v", "negative", "byteless", "other_row", "past_n", "push", "pop0", "limit"]
BASES = [-1, MASK_BODY, MASK_BODY, -1, MASK_FIRST]
assert math.gcd(len(STATES), len(PENDS)) == 1
# rows that the 64-row cases hold whatever the cycle gives: (state kind, pending mode)
FORCED = [(STATES.index((J, K + b"1", None)), "pop0"), (STATES.index((J, K + b"[" * 6, None)), "limit"),
          (1, "push"), (STATES.index((J, K + b"[" * 63, None)), "push"), (STATES.index((J, K + b"[" * 15, None)), "none"),
          (STATES.index((J, K + b"[" * 62, None)), "none"), (STATES.index((S, b'{"a":[],"x":[{"q":[', None)), "push")]


def pack(stack) -> np.ndarray:
    w = [0] * 8
    for i, y in enumerate(stack):
        w[i // 8] |= y << (4 * (i % 8))
    return np.asarray(w, dtype=np.uint32)


@dataclass
class Case:
    V: int
    rows: int
    vocab: list
    eos_ids: tuple
    trans: np.ndarray
    accept: np.ndarray
    pop: np.ndarray
    row_base: np.ndarray
    row_nstates: np.ndarray
    row_state: np.ndarray
    row_kind: np.ndarray
    row_depth: np.ndarray
    row_stack: np.ndarray
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


def _walk(g, s, stack, data):
    if isinstance(g, guided.StackGuide):
        return g.walk(s, data, stack)
    return g.walk(s, data), ()


def make_case(V: int, rows: int, with_base: bool, with_pend: bool = True, shift: int = 0, forced=()) -> Case:
    vocab, eos_ids = vocabulary(V)
    trans, accept, pop, bases = arena()
    gs = guides()
    n_tok = rows + 2
    row_base = np.full(rows, -1, dtype=np.int32)
    row_n = np.zeros(rows, dtype=np.int32)
    row_state = np.zeros(rows, dtype=np.int32)
    row_kind = np.zeros(rows, dtype=np.int32)
    row_depth = np.zeros(rows, dtype=np.int32)
    row_stack = np.zeros((rows, 8), dtype=np.uint32)
    pend = np.full(rows, -1, dtype=np.int32)
    tokens = np.zeros(n_tok, dtype=np.int32)
    base_idx = np.full(rows, -1, dtype=np.int32)
    kinds: list = [None] * rows
    k = shift
    forced = list(forced)
    for r in range(rows):
        base_idx[r] = BASES[(r + shift) % len(BASES)]
        if rows > 1 and r % 3 == 0:   # not guided; the stack fields of such a row are garbage on purpose
            tokens[r] = (r * 37) % V
            row_kind[r], row_depth[r], row_stack[r] = r % 2, 70 - r, 0x12345678
            continue
        if forced:
            ki, mode = forced.pop(0)
        else:
            ki, mode = k % len(STATES), PENDS[k % len(PENDS)]
            k += 1
        gi, lead, tweak = STATES[ki]
        g = gs[gi]
        s, stack = (g.walk(0, lead, (), per_token=False) if gi != A else (g.walk(0, lead), ()))
        assert s >= 0
        stack = list(stack)
        row_base[r], row_n[r], row_state[r] = bases[gi], g.nstates, s
        row_kind[r] = 0 if gi == A else 1
        row_depth[r] = len(stack)
        row_stack[r] = pack(stack)
        if gi == A:   # a DFA row ignores the stack fields
            row_depth[r], row_stack[r] = 99, 0xFFFFFFFF
        if tweak == "empty":
            stack = []
            row_depth[r], row_stack[r] = 0, 0
        elif tweak == "depth65":
            row_depth[r], row_stack[r] = 65, 0x33333333
        elif tweak == "depth-1":
            row_depth[r] = -1
        elif tweak == "sym0":
            row_stack[r] &= ~np.uint32(0xF0)      # symbol 1 of 3 becomes 0
        dead = tweak in ("depth65", "depth-1", "sym0")
        pend[r] = r

        def alive(p):
            return not dead and _walk(g, s, stack, p)[0] >= 0

        def pick(pred, fallback):
            for want in (pred, fallback):
                try:
                    return _first(vocab, want)
                except StopIteration:
                    pass
            return _first(vocab, lambda p: True)

        if mode == "none":
            pend[r] = -1
        elif mode == "live":
            tokens[r] = pick(alive, lambda p: True)
        elif mode == "kill":
            tokens[r] = pick(lambda p: not alive(p), lambda p: True)
        elif mode == "eos":
            tokens[r] = eos_ids[r % 2]
        elif mode == "past_v":
            tokens[r] = V + r
        elif mode == "negative":
            tokens[r] = -1 - r
        elif mode == "byteless":
            tokens[r] = 3
        elif mode == "other_row":
            pend[r] = (r + 1) % n_tok if rows > 1 else rows
        elif mode == "past_n":
            pend[r] = n_tok + r
        elif mode == "push":      # a live token that leaves the stack deeper; at depth 64 the push kills
            tokens[r] = pick(lambda p: alive(p) and len(_walk(g, s, stack, p)[1]) > len(stack),
                             lambda p: p[:1] in (b"[", b"{"))
        elif mode == "pop0":      # a live token that empties a stack that was not empty
            tokens[r] = pick(lambda p: bool(stack) and alive(p) and not _walk(g, s, stack, p)[1], alive)
        elif mode == "limit":     # dies on the 17th live push of one token
            tokens[r] = pick(lambda p: p == P17, lambda p: not alive(p))
        kinds[r] = ki, mode
    tokens[rows] = _first(vocab, lambda p: p in (b"{", b"["))
    tokens[rows + 1] = V - 1
    bits = build_masks(Tok(vocab, eos_ids)) if with_base else None
    return Case(V, rows, vocab, eos_ids, trans, accept, pop, row_base, row_n, row_state, row_kind, row_depth,
                row_stack, pend if with_pend else None, tokens if with_pend else None, bits,
                base_idx if with_base else None, kinds)


VS = (31, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 128256)


def _cases():
    out = []
    shift = 0
    for V in VS:
        for rows in (1, 3, 64):
            if rows == 64 and V > 2 * TILE + 1:
                continue   # the literal reference stays within seconds
            if rows == 1 and V == 128256:
                # one row at the large vocabulary: a deep stack row with many live tokens
                out.append(make_case(V, 1, with_base=False, forced=[(STATES.index((J, K + b"[" * 15, None)), "live")]))
                continue
            out.append(make_case(V, rows, with_base=rows != 1, shift=shift, forced=FORCED if rows == 64 else ()))
            shift += 5
    out += [make_case(V, 1, True, shift=V) for V in (31, 65, TILE + 1)]
    out += [make_case(TILE - 1, 3, False, shift=1), make_case(65, 3, True, with_pend=False, shift=2),
            make_case(TILE + 1, 64, False, with_pend=False, shift=3),
            make_case(2 * TILE + 1, 64, True, shift=9), make_case(TILE, 64, True, shift=17)]
    return out


CASES = _cases()


def literal_uncached(c: Case):
    """-> (bits uint32 [n_static + rows, words], idx, state_after, depth_after int32 [rows], stack_after uint32 [rows, 8])."""
    V, R = c.V, c.rows
    words = (V + 31) // 32
    n_static = 0 if c.base_bits is None else int(c.base_bits.shape[0])
    bits = [[0] * words for _ in range(n_static + R)]
    for i in range(n_static):
        bits[i] = [int(x) for x in c.base_bits[i]]
    idx, after, depth_after = [-1] * R, [-1] * R, [0] * R
    stack_after = [[0] * 8 for _ in range(R)]
    table = c.trans.tolist()
    pops = c.pop.tolist()
    n_tokens = 0 if c.tokens is None else len(c.tokens)
    for r in range(R):
        b0 = int(c.row_base[r])
        if b0 < 0:
            idx[r] = int(c.base_idx[r]) if c.base_idx is not None else -1
            continue
        idx[r] = n_static + r
        n = int(c.row_nstates[r])
        s = int(c.row_state[r])
        stacked = int(c.row_kind[r]) == 1
        stack: list = []
        if stacked:
            d = int(c.row_depth[r])
            if d < 0 or d > 64:
                s = -1
            else:
                stack = [(int(c.row_stack[r][i // 8]) >> (4 * (i % 8))) & 15 for i in range(d)]
                if 0 in stack or 15 in stack:
                    s, stack = -1, []

        def token(state: int, stk: list, data: bytes):
            """One token from (state, stk) -> (state, stk), or (-1, []) when it dies."""
            stk = list(stk)
            mine = 0
            for byte in data:
                e = table[b0 + state][byte]
                if not stacked:
                    if e >= n:
                        return -1, []
                    state = e
                    continue
                if e == 0xFFFF:
                    return -1, []
                sym = (e >> 11) & 15
                if e >> 15:
                    if sym != 0 or not stk:
                        return -1, []
                    state = pops[b0][stk.pop()]
                    mine = mine - 1 if mine else 0
                else:
                    state = e & 2047
                    if sym == 15:
                        return -1, []
                    if sym:
                        if len(stk) == 64 or mine == 16:
                            return -1, []
                        stk.append(sym)
                        mine += 1
                if state >= n:
                    return -1, []
            return state, stk

        ps = int(c.pend_src[r]) if c.pend_src is not None else -1
        if 0 <= ps < n_tokens and s >= 0:
            t = int(c.tokens[ps])
            if t in c.eos_ids:
                pass
            elif t < 0 or t >= V or not c.vocab[t]:
                s, stack = -1, []
            else:
                s, stack = token(s, stack, c.vocab[t])
        after[r] = s
        if stacked and s >= 0:
            depth_after[r] = len(stack)
            stack_after[r] = [int(x) for x in pack(stack)]
        base_row = None
        if c.base_bits is not None and c.base_idx[r] >= 0:
            base_row = bits[int(c.base_idx[r])]
        count = 0
        for t in range(V):
            ok = t in c.eos_ids and s >= 0 and bool(c.accept[b0 + s])
            data = c.vocab[t]
            if not ok and data and s >= 0:
                ok = token(s, stack, data)[0] >= 0
            if ok and base_row is not None:
                ok = bool((base_row[t >> 5] >> (t & 31)) & 1)
            if ok:
                bits[n_static + r][t >> 5] |= 1 << (t & 31)
                count += 1
        if count == 0:
            e0 = c.eos_ids[0]
            bits[n_static + r][e0 >> 5] |= 1 << (e0 & 31)
    return (np.asarray(bits, dtype=np.uint32).reshape(n_static + R, words), np.asarray(idx, dtype=np.int32),
            np.asarray(after, dtype=np.int32), np.asarray(depth_after, dtype=np.int32),
            np.asarray(stack_after, dtype=np.uint32).reshape(R, 8))


def literal(c: Case):
    """The literal reference, computed once per case and shared (read-only arrays)."""
    if c._literal is None:
        c._literal = literal_uncached(c)
        for a in c._literal:
            a.setflags(write=False)
    return c._literal


def _bit(row, t) -> bool:
    return bool((int(row[t >> 5]) >> (t & 31)) & 1)


def check_preconditions():
    """What the cases promise (module docstring), asserted on the cases themselves."""
    gs = guides()
    trans, accept, pop, bases = arena()
    assert len(set(bases)) == 3 and all(isinstance(g, guided.StackGuide) for g in gs[:2])
    assert gs[1].pop_to[4] < gs[1].nstates        # the schema guide has a free-form position (a symbol of its own)
    assert {c.V for c in CASES} == set(VS) and {c.rows for c in CASES} == {1, 3, 64}
    for V in VS:
        vocab, eos = vocabulary(V)
        assert len(eos) == 2 and all(vocab[e] is None for e in eos) and vocab[3] is None
        if V >= 520:
            have = {p for p in vocab if p}
            assert {bytes([x]) for x in range(256)} <= have and set(LIVE) <= have
            assert {16, 17, 40} <= {len(p) for p in have}
    seen_depth, seen_pend, seen_base, seen_kind, seen_tweak = set(), set(), set(), set(), set()
    limit_sides, row_pop, pushed, popped0, died_on_limit, nonempty = set(), 0, 0, 0, 0, set()
    for c in CASES:
        bits, idx, after, depth_after, stack_after = literal(c)
        n_static = 0 if c.base_bits is None else c.base_bits.shape[0]
        tok_id = {p: i for i, p in reversed(list(enumerate(c.vocab))) if p}
        for r, kind in enumerate(c.kinds):
            if kind is None:
                assert c.row_base[r] < 0 and after[r] == -1 and depth_after[r] == 0 and not stack_after[r].any()
                continue
            gi, lead, tweak = STATES[kind[0]]
            seen_kind.add(kind[0])
            seen_tweak.add(tweak)
            if c.pend_src is not None:
                seen_pend.add(kind[1])
            seen_base.add("none" if c.base_idx is None else int(c.base_idx[r]))
            row = bits[n_static + r]
            if tweak in ("depth65", "depth-1", "sym0"):
                e0 = c.eos_ids[0]
                assert after[r] == -1 and int(np.count_nonzero(row)) == 1 and row[e0 >> 5] == 1 << (e0 & 31)
                continue
            if gi == A or tweak:
                continue
            d = int(c.row_depth[r])
            seen_depth.add(d)
            unmasked = c.base_bits is None or c.base_idx[r] < 0
            mode = kind[1] if c.pend_src is not None else "none"
            if mode == "none" and unmasked:
                if after[r] >= 0 and np.unpackbits(row.view(np.uint8)).sum() >= 2:
                    nonempty.add(kind[0])
                if lead.endswith(b"[") and gi == J and c.V >= 520:
                    # 16 live pushes of one token pass (while the stack has room), 17 never do
                    assert _bit(row, tok_id[P16]) == (d + 16 <= 64) and not _bit(row, tok_id[P17])
                    assert _bit(row, tok_id[P16 + b"]" * 24]) == (d + 16 <= 64 and d >= 8 + 1)
                    assert not _bit(row, tok_id[P17 + b"]" * 23]) and _bit(row, tok_id[TURN]) == (d + 1 <= 64)
                    if d + 16 <= 64:
                        limit_sides |= {16, 17}
                    if d >= 2 and b"[]]" in tok_id and _bit(row, tok_id[b"[]]"]) and _bit(row, tok_id[b"]]"]):
                        row_pop += 1      # the second `]` takes a symbol of the row's stack
            if mode == "push" and after[r] >= 0 and depth_after[r] > d:
                pushed += 1
            if mode == "push" and d == 64:
                assert after[r] == -1
            if mode == "pop0" and after[r] >= 0 and d > 0 and depth_after[r] == 0:
                popped0 += 1
            if mode == "limit" and c.tokens is not None and c.vocab[int(c.tokens[r])] == P17 and lead.endswith(b"[") \
                    and d + 17 <= 64:
                assert after[r] == -1     # the depth had room: the per-token limit killed it
                died_on_limit += 1
        if c.rows == 64:
            assert c.row_base[0] < 0 and c.row_base[63] < 0 and set(bases) <= set(c.row_base.tolist())
    assert seen_depth >= set(DEPTHS), seen_depth
    assert seen_kind == set(range(len(STATES))) and seen_pend == set(PENDS)
    assert seen_tweak == {None, "empty", "depth65", "depth-1", "sym0"}
    assert seen_base == {"none", -1, MASK_FIRST, MASK_BODY}
    assert limit_sides == {16, 17} and row_pop > 0 and pushed > 0 and popped0 > 0 and died_on_limit > 0
    # every stack state kind that can go on (all but the final states) meets a mask with several bits
    want = {i for i, (gi, lead, tweak) in enumerate(STATES) if gi != A and not tweak
            and lead not in (b"{}", b'{"a":[1,2]}')}
    assert nonempty >= want, sorted(want - nonempty)


@functools.lru_cache(maxsize=None)
def token_table(V: int, device: str = "cpu"):
    from ai_agent_kubectl_amd import ops
    vocab, eos_ids = vocabulary(V)
    return ops.token_table(vocab, eos_ids, device)


def run_ops(c: Case, device: str = "cpu"):
    """ops.guide_mask_stack on the case -> the five tensors."""
    import torch
    from ai_agent_kubectl_amd import ops

    def dev(a, view=None):
        if a is None:
            return None
        return torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view))).to(device)

    return ops.guide_mask_stack(token_table(c.V, device), dev(c.trans, np.int16), dev(c.accept), dev(c.pop, np.int16),
                                dev(c.row_base), dev(c.row_nstates), dev(c.row_state), dev(c.row_kind),
                                dev(c.row_depth), dev(c.row_stack, np.int32), dev(c.pend_src), dev(c.tokens),
                                dev(c.base_bits, np.int32), dev(c.base_idx))
