"""Guided decoding: `guided_regex` / `guided_choice` of /v1/chat/completions as a byte-level DFA, and the
host bookkeeping of what ops.guide_mask (csrc/guide_mask.hip) is fed.

Compiler.  `compile_regex` parses the pattern (dialect below), builds a Thompson NFA over bytes, partitions
the 256 byte values into classes that no transition tells apart, runs the subset construction over those
classes (states x classes, not states x 256) and trims the result; `compile_choice` builds a trie.  Both
give a `Guide`: `trans` uint16 [S, 256] (DEAD = 0xFFFF), `accept` uint8 [S], start state 0, every state
reachable from 0 and able to reach an accepting one, so "not dead" means "still a prefix of some match".
Matching is whole-string.

Dialect: literals (UTF-8 encoded), `\\` escapes of metacharacters and `\\n \\t \\r`, `.`, `\\d \\w \\s \\D \\W \\S`,
`[...]` with ranges and a leading `^`, `( )`, `(?: )`, `|`, `* + ? {m} {m,} {m,n}`; a leading `^` and a
trailing `$` are accepted and ignored.  `.`, negated classes and `\\D \\W \\S` range over the fixed universe
0x09, 0x0A, 0x0D, 0x20-0x7E (`.` without 0x0A), so an open-ended construct never emits half a UTF-8
sequence; non-ASCII characters are literals outside classes only.  Everything else is a ValueError that
names the construct and its offset.  Caps (ValueError): pattern <= 2048 characters, <= 256 choices of
1..256 bytes, <= 2048 DFA states (the construction stops when it passes the cap), and, because those bound
the result and not the work, <= 32768 NFA states after the {m,n} expansion and a budget on the set operations
of the subset construction (MAX_WORK): nested counted repetition over optional parts is refused within a
fraction of a second.  A quantifier directly after a quantifier (`a**`, `a{2}{3}`) is refused as `re` does.

Per sequence a `GuideState` keeps the DFA state after the output tokens that are final (the jump-forward
prefix included; EOS does not move it; a trailing PLACEHOLDER is not walked: the runner names its device
slot in `pend_src` and the kernel walks it).  It reads `output_ids` only, so a recompute preemption leaves
it valid.  `GuideTable` is the device arena the kernel reads: one placement per distinct guide key,
refcounted by live sequences, first fit over state ranges, idle guides evicted only when their range is
needed.

JSON mode (`response_format`, `guided_json`): a byte-level DFA cannot count brackets, so `compile_json_object` and
`compile_json_schema` give a `StackGuide`, whose entries may push or pop one of 14 stack symbols (the encoding and
the limits: class StackGuide).  Both are built directly and deterministically (JSON is LL(1)), not by subset
construction.  json_object: any RFC 8259 object, starting with `{`; whitespace (space, tab, LF, CR) where the RFC
allows it inside; strings of 0x20-0x7E, the RFC's escapes and well-formed UTF-8 (RFC 3629: no overlongs,
surrogates or code points past U+10FFFF); numbers -?(0|[1-9]\\d*)(\\.\\d+)?([eE][+-]?\\d+)?; the state after the
matching `}` accepts and has no edges.  Schemas: `type` (object, array, string, integer, number, boolean, null),
`properties` in declared order (`required` members mandatory, others may be skipped, no other keys), `items` /
`minItems` / `maxItems`, `minLength` / `maxLength` in characters (an escape counts as one), `enum` / `const` of
scalars, local non-recursive `$ref` into `$defs` / `definitions`; annotations are ignored; `{}`, `true`, an object
without `properties` and an array without `items` are free-form positions (at most 11: each needs a return symbol).
Whitespace under a schema: one optional space after `:` and `,`, nothing else outside free-form positions.  Anything
else is a ValueError that names the keyword and its JSON pointer.  Caps: 16 KiB of schema, 2048 states, 64 levels.
The stack travels beside the state: GuideState.stack, `pack_guide_stacks`, ops.guide_mask_stack
(csrc/guide_stack.hip), GuideTable.arena_pop.
"""
from __future__ import annotations

import hashlib
import json
import threading
from typing import Dict, List, Optional, Sequence as Seq

import numpy as np

from .sequence import PLACEHOLDER, SamplingParams, Sequence

DEAD = 0xFFFF
MAX_PATTERN = 2048
MAX_CHOICES = 256
MAX_CHOICE_BYTES = 256
MAX_STATES = 2048
MAX_NFA_STATES = 1 << 15
# the compiler's work budget: NFA states visited by the closures plus, per DFA state built, the closure members
# merged per byte class.  The caps above bound the result; nested counted repetition can make every one of
# a few DFA states cost tens of thousands of set operations, so the work itself is bounded too (a pattern
# past it is refused in a fraction of a second).  `[a-z]{1,2046}` needs about 30 thousand units.
MAX_WORK = 400_000
GUIDE_STATES = 8192
# stack guides (StackGuide): the entry encoding and the limits that the host walk, ops/reference.py
# `guide_mask_stack` and csrc/guide_stack.hip share
POP = 0x8000
SYM_SHIFT = 11
TARGET_MASK = 0x7FF
STACK_MAX = 64        # symbols on a row's stack
STACK_WORDS = 8       # ... packed four bits each
TOKEN_PUSHES = 16     # symbols one token may have pushed and not popped again, at any point of its walk
MAX_SYMBOL = 14
SYM_TOP, SYM_OBJ, SYM_ARR = 1, 2, 3
MAX_SCHEMA_BYTES = 16384

_UNIVERSE = sum(1 << b for b in [0x09, 0x0A, 0x0D] + list(range(0x20, 0x7F)))
_DIGIT = sum(1 << b for b in range(0x30, 0x3A))
_WORD = _DIGIT | sum(1 << b for b in list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = sum(1 << b for b in (0x20, 0x09, 0x0A, 0x0D))
_SHORT = {"d": _DIGIT, "w": _WORD, "s": _SPACE,
          "D": _UNIVERSE & ~_DIGIT, "W": _UNIVERSE & ~_WORD, "S": _UNIVERSE & ~_SPACE}
_CTRL = {"n": 0x0A, "t": 0x09, "r": 0x0D}


class Guide:
    """A compiled pattern: `key` (stable hash of the source), `trans` uint16 [S, 256], `accept` uint8 [S]."""

    __slots__ = ("key", "source", "trans", "accept")

    def __init__(self, key: str, source: str, trans: np.ndarray, accept: np.ndarray):
        self.key, self.source, self.trans, self.accept = key, source, trans, accept

    @property
    def nstates(self) -> int:
        return int(self.trans.shape[0])

    def __getstate__(self):
        return (self.key, self.source, self.trans, self.accept)

    def __setstate__(self, st):
        self.key, self.source, self.trans, self.accept = st

    def walk(self, state: int, data: bytes) -> int:
        """The state after `data` from `state`; -1: dead."""
        for b in data:
            if state < 0:
                return -1
            nxt = int(self.trans[state, b])
            state = -1 if nxt == DEAD else nxt
        return state

    def matches(self, data: bytes) -> bool:
        s = self.walk(0, data)
        return s >= 0 and bool(self.accept[s])

    def is_prefix(self, data: bytes) -> bool:
        return self.walk(0, data) >= 0


def pack_stack(stack: Seq[int]) -> np.ndarray:
    """uint32 [8]: up to 64 four-bit symbols, bottom first, symbol i in bits 4 (i mod 8) of word i / 8."""
    words = np.zeros(STACK_WORDS, dtype=np.uint32)
    for i, y in enumerate(stack):
        words[i >> 3] |= np.uint32(int(y) << (4 * (i & 7)))
    return words


class StackGuide(Guide):
    """A guide with a stack (JSON mode): `trans` entries also push and pop, `pop_to` uint16 [16] names the state
    a pop of symbol y continues in.  An entry e: 0xFFFF dead; bit 15 set: pop the top symbol y (an empty stack,
    push bits that are not 0, or pop_to[y] not below S: dead) and go to pop_to[y]; else go to bits 0-10 (not
    below S: dead) and push bits 11-14 when they are not 0 (symbols 1..14; 15, a push at depth 64 and a 17th
    live push of one token: dead).  Without push or pop entries it is the DFA with the same table."""

    __slots__ = ("pop_to",)

    def __init__(self, key: str, source: str, trans: np.ndarray, accept: np.ndarray, pop_to: np.ndarray):
        super().__init__(key, source, trans, accept)
        self.pop_to = pop_to

    def __getstate__(self):
        return (self.key, self.source, self.trans, self.accept, self.pop_to)

    def __setstate__(self, st):
        self.key, self.source, self.trans, self.accept, self.pop_to = st

    def walk(self, state: int, data: bytes, stack: Seq[int] = (), per_token: bool = True):
        """(state, stack) after the bytes of ONE token from (state, stack); (-1, ()) when dead.  per_token=False
        walks a byte string that is no token: the limit on one token's live pushes does not apply."""
        S = self.nstates
        stk = list(stack)
        own = 0            # symbols this token pushed that are still on the stack
        for b in data:
            if state < 0:
                break
            e = int(self.trans[state, b])
            y = (e >> SYM_SHIFT) & 15
            if e & POP:
                if y or not stk:
                    state = -1
                    continue
                state = int(self.pop_to[stk.pop()])
                own = max(0, own - 1)
                if state >= S:
                    state = -1
                continue
            state = e & TARGET_MASK
            if state >= S or y == 15 or (y and (len(stk) >= STACK_MAX or (per_token and own >= TOKEN_PUSHES))):
                state = -1
            elif y:
                stk.append(y)
                own += 1
        return (state, tuple(stk)) if state >= 0 else (-1, ())

    def matches(self, data: bytes) -> bool:
        s, _ = self.walk(0, data, (), per_token=False)
        return s >= 0 and bool(self.accept[s])

    def is_prefix(self, data: bytes) -> bool:
        return self.walk(0, data, (), per_token=False)[0] >= 0


# ---------------------------------------------------------------------------------------------------
# parser: pattern -> tree of ("set", mask) | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None)
class _Parser:
    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0
        self.end = len(pattern)

    def fail(self, what: str, at: Optional[int] = None):
        raise ValueError(f"guided_regex: {what} at offset {self.i if at is None else at} is not supported")

    def parse(self):
        if self.p.startswith("^"):
            self.i = 1
        if self.p.endswith("$") and self.end > self.i:
            # an anchor unless an odd number of backslashes escapes it
            j = self.end - 2
            while j >= self.i and self.p[j] == "\\":
                j -= 1
            if (self.end - 2 - j) % 2 == 0:
                self.end -= 1
        node = self.alt()
        if self.i < self.end:
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < self.end and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < self.end and self.p[self.i] not in "|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        while self.i < self.end:
            c = self.p[self.i]
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                m, n = self.braces()
            else:
                break
            if c != "{":
                self.i += 1
            if self.i < self.end and self.p[self.i] in "?+":
                self.fail("lazy quantifier" if self.p[self.i] == "?" else "possessive quantifier")
            if self.i < self.end and self.p[self.i] in "*{":
                self.fail("quantifier after a quantifier (multiple repeat)")
            return ("rep", node, m, n)
        return node

    def braces(self):
        at = self.i
        j = self.p.find("}", at, self.end)
        body = self.p[at + 1:j] if j > 0 else ""
        lo, comma, hi = body.partition(",")
        if j < 0 or not (lo.isascii() and lo.isdigit()) or (hi and not (hi.isascii() and hi.isdigit())):
            self.fail("malformed {m,n} quantifier", at)
        m = int(lo)
        n = m if not comma else (int(hi) if hi else None)
        if n is not None and n < m:
            self.fail("{m,n} quantifier with n < m", at)
        if m > MAX_STATES or (n or 0) > MAX_STATES:
            raise ValueError(f"guided_regex: the {{m,n}} quantifier at offset {at} repeats more than {MAX_STATES} times")
        self.i = j + 1
        return m, n

    def atom(self):
        c = self.p[self.i]
        at = self.i
        if c == "(":
            self.i += 1
            if self.p.startswith("?", self.i):
                if self.p.startswith("?:", self.i):
                    self.i += 2
                elif self.p[self.i + 1:self.i + 2] in ("=", "!") or self.p[self.i + 1:self.i + 3] in ("<=", "<!"):
                    self.fail("lookaround", at)
                else:
                    self.fail("group extension (?...)", at)
            node = self.alt()
            if self.i >= self.end or self.p[self.i] != ")":
                self.fail("unbalanced '('", at)
            self.i += 1
            return node
        if c == "[":
            return ("set", self.klass())
        if c == ".":
            self.i += 1
            return ("set", _UNIVERSE & ~(1 << 0x0A))
        if c == "\\":
            return self.escape()
        if c in "*+?{":
            self.fail(f"quantifier {c!r} with nothing to repeat")
        if c in "^$":
            self.fail(f"anchor {c!r} inside the pattern")
        self.i += 1
        data = c.encode("utf-8")
        if len(data) == 1:
            return ("set", 1 << data[0])
        return ("cat", [("set", 1 << b) for b in data])

    def escape(self):
        """-> ("set", mask) of the escape at self.i (outside and inside a class)."""
        at = self.i
        if self.i + 1 >= self.end:
            self.fail("trailing backslash", at)
        c = self.p[self.i + 1]
        self.i += 2
        if c in _SHORT:
            return ("set", _SHORT[c])
        if c in _CTRL:
            return ("set", 1 << _CTRL[c])
        if c.isdigit():
            self.fail("backreference" if c != "0" else "octal escape", at)
        if c in "bBAZzG":
            self.fail(f"anchor \\{c}", at)
        if c.isalnum() or not c.isascii():
            self.fail(f"escape \\{c}", at)
        return ("set", 1 << ord(c))

    def klass(self) -> int:
        at = self.i
        self.i += 1
        negate = self.p.startswith("^", self.i)
        self.i += negate
        mask, first = 0, True
        while True:
            if self.i >= self.end:
                self.fail("unterminated character class", at)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if isinstance(lo, tuple):      # a shorthand class: no ranges from it
                mask |= lo[0]
                continue
            if self.p.startswith("-", self.i) and self.i + 1 < self.end and self.p[self.i + 1] != "]":
                self.i += 1
                hi = self.class_item()
                if isinstance(hi, tuple) or hi < lo:
                    self.fail("bad range in a character class", at)
                for b in range(lo, hi + 1):
                    mask |= 1 << b
            else:
                mask |= 1 << lo
        return (_UNIVERSE & ~mask) if negate else mask

    def class_item(self):
        """-> a byte value, or (mask,) for a shorthand class."""
        c = self.p[self.i]
        if not c.isascii():
            self.fail("non-ASCII character inside a character class")
        if c == "\\":
            short = self.p[self.i + 1:self.i + 2] in _SHORT
            m = self.escape()[1]
            return (m,) if short else m.bit_length() - 1
        self.i += 1
        return ord(c)


# ---------------------------------------------------------------------------------------------------
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[tuple]] = []   # (byte set mask, target)

    def new(self) -> int:
        if len(self.eps) >= MAX_NFA_STATES:
            raise ValueError(f"guided_regex: the pattern expands to more than {MAX_NFA_STATES} NFA states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> tuple:
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            if node[1]:
                self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, inner, m, n = node
        a = b = self.new()
        for _ in range(m):
            s, e = self.build(inner)
            self.eps[b].append(s)
            b = e
        if n is None:      # star: loop on one more copy
            s, e = self.build(inner)
            out = self.new()
            self.eps[b] += [s, out]
            self.eps[e] += [s, out]
            return a, out
        out = self.new()
        for _ in range(n - m):   # optional copies, each may leave for `out`
            s, e = self.build(inner)
            self.eps[b] += [s, out]
            b = e
        self.eps[b].append(out)
        return a, out


def _byte_classes(masks) -> List[int]:
    """Partition of 0..255 into classes no mask tells apart -> one representative byte per class, and
    the class of every byte."""
    sig: Dict[tuple, int] = {}
    cls = [0] * 256
    reps: List[int] = []
    for b in range(256):
        key = tuple((m >> b) & 1 for m in masks)
        c = sig.get(key)
        if c is None:
            c = sig[key] = len(reps)
            reps.append(b)
        cls[b] = c
    return reps, cls


def _determinise(nfa: _NFA, start: int, final: int, what: str):
    n = len(nfa.eps)
    closure: List[Optional[frozenset]] = [None] * n
    work = [0]

    def spend(units: int) -> None:
        work[0] += units
        if work[0] > MAX_WORK:
            raise ValueError(f"{what}: the pattern costs more than {MAX_WORK} units of work to compile (nested or "
                             "large counted repetitions over optional parts); simplify it")

    def close(s: int) -> frozenset:
        c = closure[s]
        if c is None:
            seen, stack = {s}, [s]
            while stack:
                for t in nfa.eps[stack.pop()]:
                    if t not in seen:
                        seen.add(t)
                        stack.append(t)
                if len(seen) > MAX_WORK:
                    spend(len(seen))
            spend(len(seen))
            # only states with byte edges, and the final one, matter to a subset
            c = closure[s] = frozenset(t for t in seen if nfa.edges[t] or t == final)
        return c

    masks = sorted({m for e in nfa.edges for m, _ in e})
    reps, cls = _byte_classes(masks)
    classes_of = {m: [c for c, r in enumerate(reps) if (m >> r) & 1] for m in masks}
    d0 = close(start)
    index = {d0: 0}
    order = [d0]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        moves: Dict[int, set] = {}
        for s in order[i]:
            for m, t in nfa.edges[s]:
                ct = close(t)
                spend(len(ct) * len(classes_of[m]) + 1)
                for c in classes_of[m]:
                    moves.setdefault(c, set()).update(ct)
        row = [DEAD] * len(reps)
        for c, tgt in moves.items():
            key = frozenset(tgt)
            j = index.get(key)
            if j is None:
                j = index[key] = len(order)
                order.append(key)
                if len(order) > MAX_STATES:
                    raise ValueError(f"{what}: the pattern needs more than {MAX_STATES} DFA states")
            row[c] = j
        rows.append(row)
        i += 1
    small = np.asarray(rows, dtype=np.uint16).reshape(len(order), len(reps))
    trans = small[:, np.asarray(cls, dtype=np.int64)]
    accept = np.asarray([final in d for d in order], dtype=np.uint8)
    return trans, accept


def _trim(trans: np.ndarray, accept: np.ndarray, what: str):
    """Keep the states that are reachable from 0 and reach an accepting state; renumber, 0 stays 0."""
    S = trans.shape[0]
    live = trans != DEAD
    src = np.nonzero(live)[0].astype(np.int64)
    pairs = np.unique(src * 65536 + trans[live].astype(np.int64))   # the distinct (source, target) edges
    succ: List[List[int]] = [[] for _ in range(S)]
    pred: List[List[int]] = [[] for _ in range(S)]
    for a, b in zip((pairs >> 16).tolist(), (pairs & 0xFFFF).tolist()):
        succ[a].append(b)
        pred[b].append(a)

    def search(start, nbr) -> np.ndarray:
        seen = np.zeros(S, dtype=bool)
        seen[start] = True
        stack = list(start)
        while stack:
            for t in nbr[stack.pop()]:
                if not seen[t]:
                    seen[t] = True
                    stack.append(t)
        return seen

    reach = search([0], succ)
    co = search(np.flatnonzero(accept).tolist(), pred)
    keep = reach & co
    if not keep[0]:
        raise ValueError(f"{what}: the pattern matches nothing")
    remap = np.full(S + 1, DEAD, dtype=np.uint16)
    remap[:S][keep] = np.arange(int(keep.sum()), dtype=np.uint16)
    t = trans[keep].astype(np.int64)
    t[t == DEAD] = S
    return np.ascontiguousarray(remap[t]), np.ascontiguousarray(accept[keep])


def _key(kind: str, source: str) -> str:
    return hashlib.sha256(f"{kind}:{source}".encode("utf-8")).hexdigest()


def compile_regex(pattern: str) -> Guide:
    if not isinstance(pattern, str) or not pattern:
        raise ValueError("guided_regex: the pattern must be a non-empty string")
    if len(pattern) > MAX_PATTERN:
        raise ValueError(f"guided_regex: the pattern is {len(pattern)} characters long; at most {MAX_PATTERN} are accepted")
    try:
        tree = _Parser(pattern).parse()
        nfa = _NFA()
        start, final = nfa.build(tree)
    except RecursionError:
        raise ValueError("guided_regex: the pattern nests groups too deeply") from None
    trans, accept = _trim(*_determinise(nfa, start, final, "guided_regex"), "guided_regex")
    return Guide(_key("regex", pattern), pattern, trans, accept)


def compile_choice(choices: Seq[str]) -> Guide:
    if not isinstance(choices, (list, tuple)) or not choices:
        raise ValueError("guided_choice: a non-empty list of strings is required")
    if len(choices) > MAX_CHOICES:
        raise ValueError(f"guided_choice: {len(choices)} choices; at most {MAX_CHOICES} are accepted")
    rows: List[Dict[int, int]] = [{}]
    accept = [0]
    for c in choices:
        data = c.encode("utf-8") if isinstance(c, str) else b""
        if not 1 <= len(data) <= MAX_CHOICE_BYTES:
            raise ValueError(f"guided_choice: every choice must be a string of 1..{MAX_CHOICE_BYTES} bytes")
        s = 0
        for b in data:
            t = rows[s].get(b)
            if t is None:
                t = rows[s][b] = len(rows)
                rows.append({})
                accept.append(0)
                if len(rows) > MAX_STATES:
                    raise ValueError(f"guided_choice: the choices need more than {MAX_STATES} DFA states")
            s = t
        accept[s] = 1
    trans = np.full((len(rows), 256), DEAD, dtype=np.uint16)
    for s, row in enumerate(rows):
        for b, t in row.items():
            trans[s, b] = t
    source = json.dumps(list(choices), ensure_ascii=False)
    trans, acc = _trim(trans, np.asarray(accept, dtype=np.uint8), "guided_choice")
    return Guide(_key("choice", source), source, trans, acc)


# ---------------------------------------------------------------------------------------------------
# JSON mode: direct deterministic construction (JSON is LL(1)), back to front: a value is built for a
# continuation state whose row is complete, because a number ends by lookahead and its end states take the
# continuation's edges.
_WS = b" \t\n\r"
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdefABCDEF"
_PLAIN = bytes(b for b in range(0x20, 0x7F) if b not in b'"\\')
_ANY = ("object", "array", "string", "number", "boolean", "null")


class _Builder:
    def __init__(self, what: str):
        self.what = what
        self.rows: List[List[int]] = []
        self.acc: List[int] = []
        self.pop_to = [DEAD] * 16
        self.generic: Optional[tuple] = None
        self.symbols = SYM_ARR

    def new(self, accept: bool = False) -> int:
        if len(self.rows) >= MAX_STATES:
            raise ValueError(f"{self.what}: the pattern needs more than {MAX_STATES} DFA states")
        self.rows.append([DEAD] * 256)
        self.acc.append(1 if accept else 0)
        return len(self.rows) - 1

    def edge(self, s: int, byts, t: int, push: int = 0) -> None:
        for b in byts:
            self.rows[s][b] = t | (push << SYM_SHIFT)

    def pop(self, s: int, byts) -> None:
        for b in byts:
            self.rows[s][b] = POP

    def inherit(self, s: int, cont: int) -> None:
        """`s` ends by lookahead: where it has no edge of its own it behaves as `cont`."""
        row, other = self.rows[s], self.rows[cont]
        for b in range(256):
            if row[b] == DEAD:
                row[b] = other[b]
        self.acc[s] |= self.acc[cont]

    def copy(self, src: int) -> int:
        s = self.new(bool(self.acc[src]))
        self.rows[s] = list(self.rows[src])
        return s

    def spaced(self, v: int, into: Optional[int] = None) -> int:
        """A state that takes one optional space and then behaves as `v`."""
        s = self.new() if into is None else into
        self.rows[s] = list(self.rows[v])
        self.acc[s] = self.acc[v]
        self.edge(s, b" ", v)
        return s

    # ---- scalars ----
    def chars(self, s: int, nxt: int) -> None:
        """One string character from `s` to `nxt`: a plain one, an escape, or well-formed UTF-8 (RFC 3629)."""
        new, edge = self.new, self.edge
        edge(s, _PLAIN, nxt)
        esc, h0, h1, h2, h3 = new(), new(), new(), new(), new()
        edge(s, b"\\", esc)
        edge(esc, b'"\\/bfnrt', nxt)
        edge(esc, b"u", h0)
        for a, b in ((h0, h1), (h1, h2), (h2, h3), (h3, nxt)):
            edge(a, _HEX, b)
        u1, u2, u3, e0, ed, f0, f4 = new(), new(), new(), new(), new(), new(), new()
        cont = range(0x80, 0xC0)
        edge(u1, cont, nxt)
        edge(u2, cont, u1)
        edge(u3, cont, u2)
        edge(s, range(0xC2, 0xE0), u1)
        edge(s, [0xE0], e0)
        edge(e0, range(0xA0, 0xC0), u1)
        edge(s, list(range(0xE1, 0xED)) + [0xEE, 0xEF], u2)
        edge(s, [0xED], ed)
        edge(ed, range(0x80, 0xA0), u1)
        edge(s, [0xF0], f0)
        edge(f0, range(0x90, 0xC0), u2)
        edge(s, range(0xF1, 0xF4), u3)
        edge(s, [0xF4], f4)
        edge(f4, range(0x80, 0x90), u2)

    def string(self, end: int, lo: int = 0, hi: Optional[int] = None) -> int:
        """-> the state after the opening quote of a string of lo..hi characters whose closing quote leads to `end`."""
        n = (lo if hi is None else hi) + 1
        body = [self.new() for _ in range(n)]
        for c, s in enumerate(body):
            if c >= lo:
                self.edge(s, b'"', end)
            if hi is None or c < hi:
                self.chars(s, body[c + 1] if c + 1 < n else s)
        return body[0]

    def number(self, st: int, cont: int, integer: bool = False) -> None:
        """-?(0|[1-9]\\d*)(\\.\\d+)?([eE][+-]?\\d+)? from `st`; the end states continue as `cont`."""
        new, edge = self.new, self.edge
        neg, zero, intd = new(), new(), new()
        for s in (st, neg):
            edge(s, b"0", zero)
            edge(s, b"123456789", intd)
        edge(st, b"-", neg)
        edge(intd, _DIGITS, intd)
        ends = [zero, intd]
        if not integer:
            dot, frac, e, sign, exp = new(), new(), new(), new(), new()
            for s in (zero, intd, frac):
                edge(s, b"eE", e)
            edge(zero, b".", dot)
            edge(intd, b".", dot)
            edge(dot, _DIGITS, frac)
            edge(frac, _DIGITS, frac)
            edge(e, b"+-", sign)
            for s in (e, sign, exp):
                edge(s, _DIGITS, exp)
            ends += [frac, exp]
        for s in ends:
            self.inherit(s, cont)

    def word(self, st: int, text: bytes, cont: int) -> None:
        for i, b in enumerate(text):
            nxt = cont if i == len(text) - 1 else self.new()
            self.edge(st, [b], nxt)
            st = nxt

    # ---- the free-form value ----
    def containers(self) -> tuple:
        """The generic container states, built once: (after `{`, after `[`).  A `{` or `[` inside pushes the kind
        of the enclosing container, a close pops it and continues after that container's value."""
        if self.generic is None:
            new, edge = self.new, self.edge
            obj_open, obj_next, after_key, val_o, avo, val_a, arr_open, ava = (new() for _ in range(8))
            self.generic = (obj_open, arr_open)
            for s in (obj_open, obj_next, after_key, val_o, avo, val_a, ava):
                edge(s, _WS, s)
            edge(avo, b",", obj_next)
            self.pop(avo, b"}")
            edge(ava, b",", val_a)
            self.pop(ava, b"]")
            self.pop_to[SYM_OBJ], self.pop_to[SYM_ARR] = avo, ava
            key = self.string(after_key)
            edge(obj_open, b'"', key)
            self.pop(obj_open, b"}")
            edge(obj_next, b'"', key)
            edge(after_key, b":", val_o)
            self.free_into(val_o, avo, SYM_OBJ, _ANY)
            self.free_into(val_a, ava, SYM_ARR, _ANY)
            self.rows[arr_open] = list(self.rows[val_a])
            edge(arr_open, _WS, arr_open)
            self.pop(arr_open, b"]")
        return self.generic

    def free_into(self, st: int, cont: int, sym: int, kinds) -> None:
        """The first bytes of a free-form value of `kinds` on `st`; scalars continue in `cont`, containers push `sym`."""
        if "object" in kinds or "array" in kinds:
            obj_open, arr_open = self.containers()
            if "object" in kinds:
                self.edge(st, b"{", obj_open, sym)
            if "array" in kinds:
                self.edge(st, b"[", arr_open, sym)
        if "string" in kinds:
            self.edge(st, b'"', self.string(cont))
        if "number" in kinds:
            self.number(st, cont)
        if "boolean" in kinds:
            self.word(st, b"true", cont)
            self.word(st, b"false", cont)
        if "null" in kinds:
            self.word(st, b"null", cont)

    def free(self, cont: int, kinds, ptr: str) -> int:
        """A free-form position: a value start state that returns to `cont` through a symbol of its own."""
        if self.symbols >= MAX_SYMBOL:
            raise ValueError(f"{self.what}: the free-form position at {ptr or '/'} is one too many: at most "
                             f"{MAX_SYMBOL - SYM_ARR} fit (stack symbols)")
        self.symbols += 1
        self.pop_to[self.symbols] = cont
        st = self.new()
        self.free_into(st, cont, self.symbols, kinds)
        return st

    def finish(self, kind: str, source: str, start: int) -> StackGuide:
        """Renumber so that `start` is state 0."""
        S = len(self.rows)
        trans = np.asarray(self.rows, dtype=np.uint16).reshape(S, 256)
        accept = np.asarray(self.acc, dtype=np.uint8)
        pop_to = np.asarray(self.pop_to, dtype=np.uint16)
        if start != 0:
            perm = np.arange(S)
            perm[[0, start]] = [start, 0]       # its own inverse
            trans, accept = trans[perm], accept[perm]
            goes = (trans & POP) == 0
            tgt = trans & TARGET_MASK
            ok = goes & (tgt < S)
            trans[ok] = (trans[ok] & ~np.uint16(TARGET_MASK)) | perm[tgt[ok]].astype(np.uint16)
            live = pop_to < S
            pop_to[live] = perm[pop_to[live]].astype(np.uint16)
        return StackGuide(_key(kind, source), source, np.ascontiguousarray(trans), accept, pop_to)


def compile_json_object() -> StackGuide:
    """Any RFC 8259 object: `response_format: {"type": "json_object"}`.  The content starts with `{`; the state
    after the matching `}` accepts and has no edges."""
    b = _Builder("json_object")
    start, final = b.new(), b.new(accept=True)
    obj_open, _ = b.containers()
    b.edge(start, b"{", obj_open, SYM_TOP)
    b.pop_to[SYM_TOP] = final
    return b.finish("json_object", "", start)


_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$defs", "definitions", "$id", "$comment"}
_KEYWORDS = {"type", "properties", "required", "items", "minItems", "maxItems", "minLength", "maxLength", "enum",
             "const", "$ref", "additionalProperties"}
_TYPES = ("object", "array", "string", "integer", "number", "boolean", "null")


def _esc(name: str) -> str:
    return name.replace("~", "~0").replace("/", "~1")


class _Schema:
    def __init__(self, root):
        self.root = root
        self.b = _Builder("guided_json")

    def fail(self, what: str, ptr: str):
        raise ValueError(f"guided_json: {what} at {ptr or '/'} is not supported")

    def count(self, sch, name: str, ptr: str) -> Optional[int]:
        v = sch.get(name)
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
            raise ValueError(f"guided_json: '{name}' at {ptr}/{name} must be a non-negative integer")
        return v

    def value(self, sch, ptr: str, cont: int, refs: tuple = ()) -> int:
        """-> the start state of a value under `sch` that continues in `cont` (whose row is complete)."""
        b = self.b
        if sch is True:
            return b.free(cont, _ANY, ptr)
        if not isinstance(sch, dict):
            raise ValueError(f"guided_json: the schema at {ptr or '/'} must be an object")
        for kw in sch:
            if kw not in _KEYWORDS and kw not in _ANNOTATIONS:
                self.fail(f"'{kw}'", f"{ptr}/{_esc(kw)}")
        if sch.get("additionalProperties", False) is not False:
            self.fail("'additionalProperties' other than false", f"{ptr}/additionalProperties")
        if "$ref" in sch:
            ref = sch["$ref"]
            parts = ref.split("/") if isinstance(ref, str) else []
            if len(parts) != 3 or parts[0] != "#" or parts[1] not in ("$defs", "definitions") \
                    or not isinstance(self.root.get(parts[1]), dict) \
                    or parts[2].replace("~1", "/").replace("~0", "~") not in self.root[parts[1]]:
                self.fail(f"'$ref' {ref!r} (only #/$defs/NAME and #/definitions/NAME)", f"{ptr}/$ref")
            if ref in refs:
                self.fail(f"a recursive '$ref' {ref!r}", f"{ptr}/$ref")
            target = self.root[parts[1]][parts[2].replace("~1", "/").replace("~0", "~")]
            return self.value(target, ref[1:], cont, refs + (ref,))
        if "enum" in sch or "const" in sch:
            return self.enum(sch["enum"] if "enum" in sch else [sch["const"]], f"{ptr}/{'enum' if 'enum' in sch else 'const'}", cont)
        t = sch.get("type")
        if isinstance(t, list):
            self.fail("a list of types", f"{ptr}/type")
        if t is None:
            t = "object" if "properties" in sch else "array" if "items" in sch else None
            if t is None:
                if any(k in _KEYWORDS for k in sch if k != "additionalProperties"):
                    self.fail("a schema without 'type'", ptr)
                return b.free(cont, _ANY, ptr)
        if t not in _TYPES:
            self.fail(f"type {t!r}", f"{ptr}/type")
        if t == "object":
            if "properties" not in sch:
                if sch.get("required"):
                    self.fail("'required' without 'properties'", f"{ptr}/required")
                return b.free(cont, ("object",), ptr)
            return self.object(sch, ptr, cont, refs)
        if t == "array":
            if "items" not in sch:
                return b.free(cont, ("array",), ptr)
            return self.array(sch, ptr, cont, refs)
        st = b.new()
        if t == "string":
            lo, hi = self.count(sch, "minLength", ptr) or 0, self.count(sch, "maxLength", ptr)
            if hi is not None and hi < lo:
                raise ValueError(f"guided_json: 'maxLength' at {ptr}/maxLength is below minLength")
            b.edge(st, b'"', b.string(cont, lo, hi))
        elif t in ("integer", "number"):
            b.number(st, cont, integer=t == "integer")
        elif t == "boolean":
            b.word(st, b"true", cont)
            b.word(st, b"false", cont)
        else:
            b.word(st, b"null", cont)
        return st

    def enum(self, values, ptr: str, cont: int) -> int:
        b = self.b
        if not isinstance(values, list) or not values:
            raise ValueError(f"guided_json: 'enum' at {ptr} must be a non-empty list")
        trie: dict = {}
        for v in values:
            if not (v is None or isinstance(v, (str, int, float, bool))) or (isinstance(v, float) and v != v) \
                    or v in (float("inf"), float("-inf")):
                self.fail("a value that is not a scalar", ptr)
            node = trie
            for byte in json.dumps(v, ensure_ascii=False).encode("utf-8"):
                node = node.setdefault(byte, {})
            node[-1] = True      # a spelling ends here

        def emit(node) -> int:
            s = b.new()
            for byte, child in node.items():
                if byte >= 0:
                    b.edge(s, [byte], cont if len(child) == 1 and -1 in child else emit(child))
            if -1 in node:
                b.inherit(s, cont)
            return s

        return emit(trie)

    def object(self, sch, ptr: str, cont: int, refs: tuple) -> int:
        b = self.b
        props = sch["properties"]
        required = sch.get("required", [])
        if not isinstance(props, dict) or not isinstance(required, list):
            raise ValueError(f"guided_json: 'properties' at {ptr}/properties must be an object and 'required' a list")
        names = list(props)
        for r in required:
            if r not in props:
                raise ValueError(f"guided_json: 'required' at {ptr}/required names {r!r}, which 'properties' lacks")
        n = len(names)
        need = [name in required for name in names]
        after_key = [0] * n
        after = cont          # the state after member j (before the members from j + 1 on)
        for j in range(n, -1, -1):
            if j < n:
                v = self.value(props[names[j]], f"{ptr}/properties/{_esc(names[j])}", after, refs)
                after_key[j] = b.new()
                b.edge(after_key[j], b":", b.spaced(v))
            # the members that may come next: j, and those behind optional ones
            cands = []
            for k in range(j, n):
                cands.append(k)
                if need[k]:
                    break
            closable = not any(need[j:])
            st = b.new()
            if cands:
                trie: dict = {}
                for k in cands:
                    node = trie
                    for byte in json.dumps(names[k], ensure_ascii=False).encode("utf-8")[1:]:
                        node = node.setdefault(byte, {})
                    node[-1] = k

                def emit(node) -> int:
                    s = b.new()
                    for byte, child in node.items():
                        b.edge(s, [byte], after_key[child[-1]] if -1 in child else emit(child))
                    return s

                quote = b.new()
                b.edge(quote, b'"', emit(trie))
                if j == 0:
                    b.rows[st] = list(b.rows[quote])
                else:
                    b.edge(st, b",", b.spaced(quote))
            if closable:
                b.edge(st, b"}", cont)
            after = st
        start = b.new()
        b.edge(start, b"{", after)
        return start

    def array(self, sch, ptr: str, cont: int, refs: tuple) -> int:
        b = self.b
        lo, hi = self.count(sch, "minItems", ptr) or 0, self.count(sch, "maxItems", ptr)
        if hi is not None and hi < lo:
            raise ValueError(f"guided_json: 'maxItems' at {ptr}/maxItems is below minItems")
        items, iptr = sch["items"], f"{ptr}/items"
        start = b.new()
        if hi == 0:
            last = b.new()
            b.edge(last, b"]", cont)
            b.edge(start, b"[", last)
            return start
        top = hi if hi is not None else max(lo, 1)
        after = b.new()                       # after `top` items
        b.edge(after, b"]", cont)
        if hi is None:                        # ... any number more
            comma = b.new()
            b.edge(after, b",", comma)
            b.spaced(self.value(items, iptr, after, refs), into=comma)
        for k in range(top - 1, 0, -1):       # after k items
            st = b.new()
            b.edge(st, b",", b.spaced(self.value(items, iptr, after, refs)))
            if k >= lo:
                b.edge(st, b"]", cont)
            after = st
        first = b.copy(self.value(items, iptr, after, refs))
        if lo == 0:
            b.edge(first, b"]", cont)
        b.edge(start, b"[", first)
        return start


def compile_json_schema(schema) -> StackGuide:
    """`response_format: {"type": "json_schema"}` / `guided_json`: the subset of JSON Schema in the module
    docstring, as a dict or a JSON string.  ValueError names what is outside it."""
    if isinstance(schema, str):
        if len(schema.encode("utf-8")) > MAX_SCHEMA_BYTES:
            raise ValueError(f"guided_json: the schema is larger than {MAX_SCHEMA_BYTES} bytes")
        try:
            schema = json.loads(schema)
        except ValueError as e:
            raise ValueError(f"guided_json: the schema is not JSON ({e})") from None
    if schema is not True and not isinstance(schema, dict):
        raise ValueError("guided_json: the schema must be a JSON object")
    try:
        source = json.dumps(schema, ensure_ascii=False, allow_nan=False)
    except (TypeError, ValueError) as e:
        raise ValueError(f"guided_json: the schema is not JSON ({e})") from None
    if len(source.encode("utf-8")) > MAX_SCHEMA_BYTES:
        raise ValueError(f"guided_json: the schema is larger than {MAX_SCHEMA_BYTES} bytes")
    c = _Schema(schema if isinstance(schema, dict) else {})
    final = c.b.new(accept=True)
    try:
        start = c.value(schema, "", final)
    except RecursionError:
        raise ValueError("guided_json: the schema nests too deeply") from None
    return c.b.finish("json_schema", source, start)


# ---------------------------------------------------------------------------------------------------
def single_byte_tokens(tokenizer) -> np.ndarray:
    """bool [256]: some token of the vocabulary spells exactly this byte."""
    have = getattr(tokenizer, "_guided_single_bytes", None)
    if have is None:
        have = np.zeros(256, dtype=bool)
        for p in tokenizer.id_to_bytes:
            if p is not None and len(p) == 1:
                have[p[0]] = True
        try:
            tokenizer._guided_single_bytes = have
        except AttributeError:
            pass
    return have


def validate(p: SamplingParams, tokenizer, tp_size: int, forced_prefix: Optional[Seq[int]] = None) -> None:
    """Raise ValueError (HTTP 400 upstream) for a guided request this engine cannot serve."""
    g = getattr(p, "guide", None)
    if g is None:
        return
    if not isinstance(g, Guide):
        raise ValueError("guide must be a compiled Guide (engine.guided.compile_regex / compile_choice)")
    if tp_size > 1:
        # the mask is built over the whole vocabulary and the worker protocol does not carry the image
        raise ValueError("guided_regex / guided_choice / guided_json / response_format are not supported with "
                         "tensor parallelism (TP > 1)")
    if g.nstates > MAX_STATES:
        raise ValueError(f"guide holds {g.nstates} states; at most {MAX_STATES} are accepted")
    spell = ((g.trans != DEAD) & single_byte_tokens(tokenizer)[None, :]).any(axis=1) | g.accept.astype(bool)
    if not spell.all():
        raise ValueError("this tokenizer cannot spell the pattern: state "
                         f"{int(np.argmin(spell))} of the guide has no continuation that a single-byte token spells")
    s, stack = 0, ()
    for t in forced_prefix or ():
        data = tokenizer.token_bytes(int(t))
        if not data:
            s = -1
        elif isinstance(g, StackGuide):
            s, stack = g.walk(s, data, stack)
        else:
            s = g.walk(s, data)
        if s < 0:
            raise ValueError("the guide does not admit the forced prefix "
                             f"{tokenizer.decode(list(forced_prefix))!r} that SAFE_DECODE starts the reply with")


class GuideState:
    """One sequence's position in its guide: `state` (local, -1 = dead) and, for a StackGuide, `stack` (the
    symbols, bottom first) after `counted` output tokens."""

    def __init__(self, seq: Sequence):
        self.guide: Guide = seq.params.guide
        self.state = 0
        self.stack: tuple = ()
        self.counted = 0

    def update(self, seq: Sequence, tokenizer) -> None:
        """Walk the bytes of the output tokens that became final since the last call."""
        out = seq.output_ids
        n = len(out) - (1 if out and out[-1] == PLACEHOLDER else 0)
        for t in out[self.counted:n]:
            if t < 0:
                raise RuntimeError(f"seq {seq.seq_id}: an unsettled token inside output_ids")
            if tokenizer.is_eos(t):
                continue
            data = tokenizer.token_bytes(t)
            if not data:
                self.state = -1
            elif isinstance(self.guide, StackGuide):
                self.state, self.stack = self.guide.walk(self.state, data, self.stack)
            else:
                self.state = self.guide.walk(self.state, data)
        self.counted = max(self.counted, n)


def state_of(seq: Sequence, tokenizer) -> GuideState:
    st = seq.guide_state
    if st is None:
        st = seq.guide_state = GuideState(seq)
    st.update(seq, tokenizer)
    return st


class Placement:
    __slots__ = ("key", "base", "nstates", "refs", "guide", "uploaded", "used", "kind")

    def __init__(self, guide: Guide, base: int, used: int):
        self.key, self.base, self.nstates, self.refs = guide.key, base, guide.nstates, 0
        self.kind = 1 if isinstance(guide, StackGuide) else 0   # ops.guide_mask_stack's row_kind
        self.guide: Optional[Guide] = guide     # dropped once uploaded
        self.uploaded = False
        self.used = used


class GuideTable:
    """Device arena int16 (the uint16 patterns) [states, 256] + uint8 [states] accept flags + int16 [states, 16]
    `arena_pop` (row `base` of a StackGuide's range holds its pop_to; every other row is dead), and the host
    allocator over its state ranges.  acquire / release may be called from any thread; `flush` uploads
    what was placed since the last call and runs on the engine's thread, on its stream, before the step
    that first reads the range: the copy is ordered behind every earlier step that read what it replaces."""

    def __init__(self, states: int = GUIDE_STATES, device="cpu"):
        import torch
        self.states = int(states)
        self.trans = torch.full((self.states, 256), -1, dtype=torch.int16, device=device)
        self.accept = torch.zeros(self.states, dtype=torch.uint8, device=device)
        self.arena_pop = torch.full((self.states, 16), -1, dtype=torch.int16, device=device)
        self.placed: Dict[str, Placement] = {}
        self._pending: List[Placement] = []
        self._lock = threading.Lock()
        self._clock = 0
        self.uploads = 0

    def _gap(self, n: int) -> int:
        at = 0
        for p in sorted(self.placed.values(), key=lambda q: q.base):
            if p.base - at >= n:
                return at
            at = p.base + p.nstates
        return at if self.states - at >= n else -1

    def acquire(self, guide: Guide) -> Placement:
        with self._lock:
            self._clock += 1
            p = self.placed.get(guide.key)
            if p is None:
                n = guide.nstates
                base = self._gap(n)
                while base < 0:
                    idle = [q for q in self.placed.values() if q.refs == 0]
                    if n > self.states or not idle:
                        raise ValueError(f"the guide table is full: no room for a guide of {n} states among "
                                         f"{self.states} (GUIDE_STATES) while {len(self.placed)} guides are in use")
                    old = min(idle, key=lambda q: q.used)
                    del self.placed[old.key]
                    if old in self._pending:
                        self._pending.remove(old)
                    base = self._gap(n)
                p = self.placed[guide.key] = Placement(guide, base, self._clock)
                self._pending.append(p)
            p.refs += 1
            p.used = self._clock
            return p

    def release(self, p: Placement) -> None:
        with self._lock:
            if p.refs > 0:
                p.refs -= 1

    def flush(self) -> None:
        import torch
        with self._lock:
            todo, self._pending = self._pending, []
        for p in todo:
            g = p.guide
            self.trans[p.base:p.base + p.nstates].copy_(torch.from_numpy(g.trans.view(np.int16)))
            self.accept[p.base:p.base + p.nstates].copy_(torch.from_numpy(g.accept))
            pop = g.pop_to if isinstance(g, StackGuide) else np.full(16, DEAD, dtype=np.uint16)
            self.arena_pop[p.base].copy_(torch.from_numpy(pop.view(np.int16)))
            p.uploaded, p.guide = True, None
            self.uploads += 1


def pack_guides(seqs: Seq[Sequence], rows: int, pend: Optional[List[int]] = None, tokenizer=None) -> np.ndarray:
    """-> the int32 image of models/llama.py GuideArrays for a step of `rows` rows (the batch, then padding):
    [base | nstates | state | pend_src] (rows each).  base: the arena base of the row's guide, -1 for a row
    that is not guided; state: the local state after the row's final output tokens (-1 = dead); pend_src: the
    d_out slot of the row's newest output token when that is still on the device, else -1.
    Every guided sequence holds its placement in `guide_ref` (engine.submit / the runner took it)."""
    img = np.zeros(4 * rows, dtype=np.int32)
    img[:rows] = -1
    img[3 * rows:] = -1
    for i, s in enumerate(seqs):
        ref = s.guide_ref
        if s.params.guide is None or ref is None:   # not guided, or it has left (its token is discarded)
            continue
        st = state_of(s, tokenizer)
        img[i] = ref.base
        img[rows + i] = ref.nstates
        img[2 * rows + i] = st.state
        if pend is not None:
            img[3 * rows + i] = pend[i]
    return img


def pack_guide_stacks(seqs: Seq[Sequence], rows: int, tokenizer=None) -> np.ndarray:
    """-> the int32 image [kind | depth | stack words] (rows, rows, 8 * rows) that ops.guide_mask_stack takes
    beside pack_guides' for a step with a StackGuide row.  kind: 1 for a row under a StackGuide, else 0; depth:
    the symbols on the row's stack after its final output tokens; stack words: row r's 64 four-bit symbols in
    words [8 r, 8 r + 8) of the last section, bottom first, symbol i in bits 4 (i mod 8) of word i / 8."""
    img = np.zeros(10 * rows, dtype=np.int32)
    words = img[2 * rows:].view(np.uint32).reshape(rows, 8)
    for i, s in enumerate(seqs):
        if not isinstance(s.params.guide, StackGuide) or s.guide_ref is None:
            continue
        st = state_of(s, tokenizer)
        img[i] = 1
        img[rows + i] = len(st.stack)
        words[i] = pack_stack(st.stack)
    return img
