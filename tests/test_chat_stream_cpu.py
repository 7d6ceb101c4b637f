"""engine/streaming.py without an engine: `StreamDecoder` releases exactly the content that `stop_cut` and one
whole-string decode define, for invalid UTF-8 too, and a token's logprob entry leaves with its first byte."""
import random

import pytest

from ai_agent_kubectl_amd.engine.streaming import StopScanner, StreamDecoder, stop_cut, validate_stops

VALID = ["a", "z", " ", "\n", "é", "ß", "€", "✓", "한", "😀", "\U0001F680"]
BROKEN = [b"\xc3", b"\xe2\x82", b"\xf0\x9f", b"\xf0\x9f\x98", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xf0\x80\x80\xaf",
          b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xff", b"\x80", b"\xbf\xbf", b"\xf8\x88\x80\x80\x80"]


def _random_bytes(rng) -> bytes:
    out = bytearray()
    for _ in range(rng.randint(0, 24)):
        out += rng.choice(VALID).encode() if rng.random() < 0.7 else rng.choice(BROKEN)
    return bytes(out)


def _pieces(rng, data: bytes):
    out, i = [], 0
    while i < len(data):
        n = rng.randint(1, 4)
        out.append(data[i:i + n])
        i += n
    return out


def _stops(rng, data: bytes):
    stops = []
    for _ in range(rng.randint(0, 4)):
        n = rng.randint(1, 8)
        if data and rng.random() < 0.3:
            at = rng.randrange(len(data))
            stops.append(data[at:at + n])
        else:
            stops.append(bytes(rng.choice(b"az \n\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80\xffq") for _ in range(n)))
    return stops


def _stream(pieces, stops):
    """Feed a completion as the engine would produce it (it ends with the token that completes a stop string) ->
    (released texts joined, released token indices, bytes released after every call, decoder)."""
    cut, _, used = stop_cut(pieces, stops)
    dec = StreamDecoder(stops or None)
    texts, tokens, marks = [], 0, []
    for p in pieces[:used]:
        text, n = dec.feed(p)
        texts.append(text)
        tokens += n
        marks.append(dec._released)
    text, n = dec.finish()
    texts.append(text)
    return "".join(texts), tokens + n, marks, dec


def test_stream_decoder_matches_the_whole_string_reference_on_random_cases():
    rng = random.Random(20240607)
    matched = 0
    for case in range(3000):
        data = _random_bytes(rng)
        pieces, stops = _pieces(rng, data), _stops(rng, data)
        cut, which, used = stop_cut(pieces, stops)
        whole = b"".join(pieces[:used])
        want = (whole if cut is None else whole[:cut]).decode("utf-8", "replace")
        got, tokens, marks, dec = _stream(pieces, stops)
        assert got == want, (case, pieces, stops)
        assert (dec.cut, dec.match) == (cut, which), (case, pieces, stops)
        # no release reaches the cut, and what was released never shrinks
        assert all(m <= (len(whole) if cut is None else cut) for m in marks) and marks == sorted(marks)
        starts = [sum(len(p) for p in pieces[:i]) for i in range(used)]
        assert tokens == sum(1 for s in starts if cut is None or s < cut), (case, pieces, stops)
        matched += cut is not None
    assert 900 < matched < 2100   # about half the cases stop


def test_entries_leave_with_the_first_byte_of_their_token():
    rng = random.Random(5)
    for _ in range(500):
        data = _random_bytes(rng)
        pieces, stops = _pieces(rng, data), _stops(rng, data)
        _, _, used = stop_cut(pieces, stops)
        dec = StreamDecoder(stops or None)
        starts, out = [], 0
        for p in pieces[:used]:
            starts.append(sum(len(x) for x in pieces[:len(starts)]))
            out += dec.feed(p)[1]
            assert out == sum(1 for s in starts if s < dec._released)
        assert dec.tokens == out


def test_scanner_agrees_with_the_brute_force_for_long_stops():
    rng = random.Random(9)
    for _ in range(500):
        data = bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 40)))
        pieces = _pieces(rng, data)
        stops = [bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 6))) for _ in range(rng.randint(1, 4))]
        sc, hit, used = StopScanner(stops), None, 0
        for p in pieces:
            used += 1
            hit = sc.feed(p)
            if hit is not None:
                break
        cut, which, n = stop_cut(pieces, stops)
        assert (hit or (None, None)) == (cut, which) and used == n


def test_a_stop_string_spanning_three_tokens():
    pieces = [b"kubectl ge", b"t po", b"ds -", b"n prod"]
    assert stop_cut(pieces, [b"e", b"get pods"]) == (3, 0, 1)   # the e of "kubectl"
    assert stop_cut(pieces, [b"et pods"]) == (9, 0, 3)
    text, tokens, marks, dec = _stream(pieces, [b"et pods"])
    assert text == "kubectl g" and marks == [9, 9, 9] and tokens == 1 and (dec.cut, dec.match) == (9, 0)


def test_a_stop_completed_inside_a_token_drops_the_tail_of_that_token():
    pieces = [b"ab", b"cd;ef", b"gh"]
    assert stop_cut(pieces, [b";"]) == (4, 0, 2)
    text, tokens, marks, _ = _stream(pieces, [b";"])
    assert text == "abcd" and tokens == 2 and marks == [2, 4]


def test_the_later_listed_stop_that_starts_earlier_wins():
    pieces = [b"x", b"abcd"]
    assert stop_cut(pieces, [b"cd", b"bc"]) == (2, 1, 2)
    assert stop_cut(pieces, [b"bc", b"bcd"]) == (2, 0, 2)   # same offset: the lowest index
    text, tokens, _, dec = _stream(pieces, [b"cd", b"bc"])
    assert text == "xa" and dec.match == 1 and tokens == 2
    # a longer string that started earlier but completes later does not count: the sequence has left by then
    assert stop_cut([b"ab", b"cd", b"ef"], [b"abcdef", b"cd"]) == (2, 1, 2)
    assert _stream([b"ab", b"cd", b"ef"], [b"abcdef", b"cd"])[0] == "ab"


def test_a_stop_equal_to_the_first_token_gives_empty_content():
    pieces = [b" get", b" pods"]
    assert stop_cut(pieces, [b" get"]) == (0, 0, 1)
    text, tokens, marks, _ = _stream(pieces, [b" get"])
    assert text == "" and tokens == 0 and marks == [0]


def test_a_dangling_half_character_at_length_is_one_replacement_character():
    pieces = [b"ok ", b"\xf0\x9f", b"\x98"]
    for stops in ([], [b"zz"]):
        dec = StreamDecoder(stops or None)
        texts = [dec.feed(p)[0] for p in pieces]
        assert texts == ["ok ", "", ""]
        text, n = dec.finish()
        assert text == "�" == b"\xf0\x9f\x98".decode("utf-8", "replace") and n == 0 and dec.tokens == 3


def test_validate_stops():
    validate_stops(None)
    validate_stops([b"a"] * 4)
    validate_stops([b"x" * 64])
    for bad in ([], [b"a"] * 5, [b""], [b"x" * 65], ["text"], b"ab"):
        with pytest.raises(ValueError):
            validate_stops(bad)
