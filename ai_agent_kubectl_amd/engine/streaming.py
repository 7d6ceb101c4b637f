"""`stop` strings and incremental detokenisation for chat completions: pure Python, no engine or torch imports.

B is the concatenation of a completion's token byte pieces (EOS has none).  A sequence with `stop` strings finishes
at the first token after which some stop string occurs in B; its cut is the smallest start offset of a match in B
at that moment (the lowest-listed string among those matching there), and its content is
B[:cut].decode("utf-8", "replace").  `stop_cut` is that definition as a brute force over whole strings;
`StopScanner` finds the same cut piece by piece (engine.py `_settle`, StreamDecoder), and `StreamDecoder` releases
text while tokens arrive such that everything released joins to exactly that content.
"""
from __future__ import annotations

import codecs
from typing import List, Optional, Sequence, Tuple

MAX_STOPS = 4
MAX_STOP_BYTES = 64


def validate_stops(stops) -> None:
    """ValueError unless `stops` is None or 1..MAX_STOPS byte strings of 1..MAX_STOP_BYTES bytes."""
    if stops is None:
        return
    if not isinstance(stops, (list, tuple)) or not 1 <= len(stops) <= MAX_STOPS:
        raise ValueError(f"stop must hold 1..{MAX_STOPS} strings")
    for s in stops:
        if not isinstance(s, (bytes, bytearray)) or not 1 <= len(s) <= MAX_STOP_BYTES:
            raise ValueError(f"every stop string must be 1..{MAX_STOP_BYTES} bytes long")


def stop_cut(pieces: Sequence[bytes], stops) -> Tuple[Optional[int], Optional[int], int]:
    """(cut, index of the matched stop string, tokens consumed) of a completion made of `pieces`; (None, None,
    len(pieces)) when no stop string ever occurs.  The reference: joins and searches the whole string per token."""
    for n in range(1, len(pieces) + 1):
        whole = b"".join(pieces[:n])
        best = None
        for i, s in enumerate(stops or ()):
            at = whole.find(s)
            if at >= 0 and (best is None or at < best[0]):
                best = (at, i)
        if best is not None:
            return best[0], best[1], n
    return None, None, len(pieces)


class StopScanner:
    """`stop_cut` one piece at a time: the search for a string s resumes len(s) - 1 bytes before the new piece."""

    __slots__ = ("stops", "buf", "hit")

    def __init__(self, stops: Sequence[bytes]):
        self.stops = [bytes(s) for s in stops]
        self.buf = bytearray()
        self.hit: Optional[Tuple[int, int]] = None   # (cut, index of the stop string)

    def feed(self, piece: bytes) -> Optional[Tuple[int, int]]:
        if self.hit is not None or not piece:
            return self.hit
        buf = self.buf
        old = len(buf)
        buf += piece
        best = None
        for i, s in enumerate(self.stops):
            at = buf.find(s, max(0, old - len(s) + 1))
            if at >= 0 and (best is None or at < best[0]):
                best = (at, i)
        self.hit = best
        return best


class StreamDecoder:
    """Fed a completion's token byte pieces in order, returns the text that is safe to release: never a byte at or
    past the cut a later piece could still set (the longest suffix of the unreleased bytes that is a proper prefix
    of a stop string is withheld), never half a character (an incremental UTF-8 decoder, errors="replace").
    `feed` and `finish` return (text, tokens): `tokens` counts the fed pieces whose first byte was released by this
    call, in feed order, so a token's log-probability entry leaves together with its first byte and an entry of a
    token that starts at or past the cut never does.  After `finish` the released text joins to
    B[:cut].decode("utf-8", "replace")."""

    def __init__(self, stops: Optional[Sequence[bytes]] = None):
        self._scan = StopScanner(stops) if stops else None
        self._longest = max((len(s) for s in stops), default=0) if stops else 0
        self._dec = codecs.getincrementaldecoder("utf-8")("replace")
        self._buf = bytearray()
        self._released = 0            # bytes handed to the decoder
        self._starts: List[int] = []  # first-byte offset of every fed piece
        self._tokens = 0              # pieces counted as released
        self.cut: Optional[int] = None
        self.match: Optional[int] = None

    @property
    def tokens(self) -> int:
        """Fed pieces whose first byte has been released."""
        return self._tokens

    def _withheld(self) -> int:
        tail = bytes(self._buf[max(self._released, len(self._buf) - self._longest + 1):])
        for k in range(len(tail), 0, -1):
            part = tail[len(tail) - k:]
            if any(len(s) > k and s.startswith(part) for s in self._scan.stops):
                return k
        return 0

    def _release(self, end: int, final: bool) -> Tuple[str, int]:
        text = self._dec.decode(bytes(self._buf[self._released:end]), final)
        self._released = max(self._released, end)
        n = self._tokens
        while n < len(self._starts) and (self._starts[n] < end or (final and self.cut is None)):
            n += 1
        n, self._tokens = n - self._tokens, n
        return text, n

    def feed(self, piece: bytes) -> Tuple[str, int]:
        if self.cut is not None:   # pieces past the token that completed a stop string are not part of the completion
            return "", 0
        self._starts.append(len(self._buf))
        self._buf += piece
        if self._scan is None:
            return self._release(len(self._buf), False)
        hit = self._scan.feed(piece)
        if hit is not None:
            self.cut, self.match = hit
            return self._release(self.cut, False)
        return self._release(len(self._buf) - self._withheld(), False)

    def finish(self) -> Tuple[str, int]:
        return self._release(len(self._buf) if self.cut is None else self.cut, True)
