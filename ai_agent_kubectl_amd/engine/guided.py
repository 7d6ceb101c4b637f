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
        raise ValueError("guided_regex / guided_choice are not supported with tensor parallelism (TP > 1)")
    if g.nstates > MAX_STATES:
        raise ValueError(f"guide holds {g.nstates} states; at most {MAX_STATES} are accepted")
    spell = ((g.trans != DEAD) & single_byte_tokens(tokenizer)[None, :]).any(axis=1) | g.accept.astype(bool)
    if not spell.all():
        raise ValueError("this tokenizer cannot spell the pattern: state "
                         f"{int(np.argmin(spell))} of the guide has no continuation that a single-byte token spells")
    s = 0
    for t in forced_prefix or ():
        s = g.walk(s, tokenizer.token_bytes(int(t))) if tokenizer.token_bytes(int(t)) else -1
        if s < 0:
            raise ValueError("the guide does not admit the forced prefix "
                             f"{tokenizer.decode(list(forced_prefix))!r} that SAFE_DECODE starts the reply with")


class GuideState:
    """One sequence's position in its guide: `state` (local, -1 = dead) after `counted` output tokens."""

    def __init__(self, seq: Sequence):
        self.guide: Guide = seq.params.guide
        self.state = 0
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
            self.state = self.guide.walk(self.state, data) if data else -1
        self.counted = max(self.counted, n)


def state_of(seq: Sequence, tokenizer) -> GuideState:
    st = seq.guide_state
    if st is None:
        st = seq.guide_state = GuideState(seq)
    st.update(seq, tokenizer)
    return st


class Placement:
    __slots__ = ("key", "base", "nstates", "refs", "guide", "uploaded", "used")

    def __init__(self, guide: Guide, base: int, used: int):
        self.key, self.base, self.nstates, self.refs = guide.key, base, guide.nstates, 0
        self.guide: Optional[Guide] = guide     # dropped once uploaded
        self.uploaded = False
        self.used = used


class GuideTable:
    """Device arena int16 (the uint16 patterns) [states, 256] + uint8 [states] accept flags, and the host
    allocator over its state ranges.  acquire / release may be called from any thread; `flush` uploads
    what was placed since the last call and runs on the engine's thread, on its stream, before the step
    that first reads the range: the copy is ordered behind every earlier step that read what it replaces."""

    def __init__(self, states: int = GUIDE_STATES, device="cpu"):
        import torch
        self.states = int(states)
        self.trans = torch.full((self.states, 256), -1, dtype=torch.int16, device=device)
        self.accept = torch.zeros(self.states, dtype=torch.uint8, device=device)
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
