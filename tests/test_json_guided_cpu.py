"""JSON mode without a GPU: the json_object and JSON Schema compilers (engine/guided.py StackGuide), the mask
definition (ops/reference.py `guide_mask_stack`) against the literal reference of tests/json_guide_cases.py, the
host bookkeeping (GuideState, GuideTable, pack_guide_stacks), the engine on the tiny CPU model and the HTTP fields."""
import json
import pickle
import random
import re
import threading

import numpy as np
import pytest
import torch

from ai_agent_kubectl_amd.engine import guided
from ai_agent_kubectl_amd.engine.sequence import PLACEHOLDER, SamplingParams, Sequence
from tests import engine_helpers
from tests import guided_cases as gc
from tests import json_guide_cases as jc

# ---------------- compile_json_object ----------------
SCALARS = [None, True, False, 0, -1, 7, 12.5, 1e10, -3.2e-5, 1e-7, 123456789012, "", "a", "é€\U0001F600", 'q"\\\n\t\x01/',
           "  x", "0", "null"]
KEYS = ["a", "b", "ké", "x y", "", 'q"k', "\U0001F600"]
STYLES = [dict(), dict(indent=2), dict(separators=(",", ":")), dict(ensure_ascii=False, indent="\t")]


def _value(rng, depth=0):
    k = rng.random()
    if depth > 3 or k < 0.45:
        return rng.choice(SCALARS)
    if k < 0.75:
        return {rng.choice(KEYS) + str(i): _value(rng, depth + 1) for i in range(rng.randint(0, 3))}
    return [_value(rng, depth + 1) for _ in range(rng.randint(0, 3))]


@pytest.fixture(scope="module")
def jobj():
    return guided.compile_json_object()


def test_json_object_accepts_json_dumps_and_keeps_every_prefix_alive(jobj):
    rng = random.Random(1)
    assert jobj.nstates <= 128 and jobj.trans.dtype == np.uint16 and jobj.pop_to.shape == (16,)
    for i in range(600):
        obj = {rng.choice(KEYS) + str(j): _value(rng) for j in range(rng.randint(0, 3))}
        for style in STYLES:
            data = json.dumps(obj, **style).encode()
            assert jobj.matches(data), data
            if i < 60:
                for n in range(len(data)):
                    s, _ = jobj.walk(0, data[:n], (), per_token=False)
                    assert s >= 0 and not jobj.accept[s], (data, n)
    final, stack = jobj.walk(0, b"{}")
    assert jobj.accept[final] and stack == () and (jobj.trans[final] == guided.DEAD).all()   # only EOS is left
    assert not jobj.is_prefix(b" {") and not jobj.is_prefix(b"[") and not jobj.is_prefix(b"{} ")


def test_json_object_accepts_exactly_the_mutations_that_parse_to_a_dict(jobj):
    """One- and two-byte mutations of json.dumps output.  The alphabet holds no `N`, `I` or `y`, so no mutation can
    spell NaN or Infinity, where Python is laxer than RFC 8259."""
    rng = random.Random(2)
    alphabet = b'{}[]",:0123456789.eE+-tfnrulsa \\\x80\xc3\xe2\xed\xf4bc\n\t\x00'
    accepted = 0
    for _ in range(6000):
        data = bytearray(json.dumps({"k": _value(rng), "z": [1, {"a": None}]}, ensure_ascii=rng.random() < 0.5).encode())
        for _ in range(rng.randint(1, 2)):
            at, op = rng.randrange(len(data)), rng.random()
            if op < 0.4:
                data[at] = rng.choice(alphabet)
            elif op < 0.7:
                del data[at]
            else:
                data.insert(at, rng.choice(alphabet))
        data = bytes(data)
        try:
            want = isinstance(json.loads(data.decode("utf-8")), dict) and data[:1] == b"{" and data[-1:] == b"}"
        except ValueError:
            want = False
        assert jobj.matches(data) == want, data
        accepted += want
    assert 300 < accepted < 3000


def test_json_object_nesting_stops_at_64(jobj):
    assert jobj.matches(b'{"a":' + b"[" * 63 + b"]" * 63 + b"}")
    s, stack = jobj.walk(0, b'{"a":' + b"[" * 63, (), per_token=False)
    assert s >= 0 and len(stack) == 64
    assert jobj.walk(s, b"[", stack) == (-1, ()) and jobj.walk(s, b"{", stack) == (-1, ())
    assert jobj.walk(s, b"1", stack)[0] >= 0
    # one token: 16 live pushes pass, the 17th dies, whatever room the stack has; popping makes room again
    s, stack = jobj.walk(0, b'{"a":[')
    assert jobj.walk(s, b"[" * 16, stack)[0] >= 0 and jobj.walk(s, b"[" * 17, stack) == (-1, ())
    assert jobj.walk(s, b"[" * 16 + b"],[", stack)[0] >= 0
    assert jobj.walk(jobj.walk(s, b"[" * 16, stack)[0], b"[", jobj.walk(s, b"[" * 16, stack)[1])[0] >= 0


def test_a_stack_guide_without_pushes_is_its_dfa_and_survives_pickling(jobj):
    g = guided.compile_regex(r"a(bc)+[d;]?")
    sg = guided.StackGuide(g.key, g.source, g.trans, g.accept, np.full(16, guided.DEAD, dtype=np.uint16))
    for data in (b"abc", b"abcbcd", b"ab", b"x", b"abcd;", b""):
        assert sg.matches(data) == g.matches(data) and sg.is_prefix(data) == g.is_prefix(data)
        assert sg.walk(0, data)[0] == g.walk(0, data)
    back = pickle.loads(pickle.dumps(jobj))
    assert isinstance(back, guided.StackGuide) and back.key == jobj.key and np.array_equal(back.pop_to, jobj.pop_to)
    assert np.array_equal(back.trans, jobj.trans) and back.matches(b'{"a":[1,{"b":null}]}')
    plain = pickle.loads(pickle.dumps(g))
    assert type(plain) is guided.Guide and plain.matches(b"abc")
    # decoding: pop with a push symbol, push 15, a target or pop_to past the states are dead
    trans = np.full((2, 256), guided.DEAD, dtype=np.uint16)
    trans[0, ord("p")] = 1 | (3 << 11)
    trans[0, ord("f")] = 1 | (15 << 11)
    trans[0, ord("t")] = 2
    trans[1, ord("q")] = guided.POP
    trans[1, ord("r")] = guided.POP | (2 << 11)
    trans[1, ord("p")] = 1 | (4 << 11)
    pop_to = np.full(16, guided.DEAD, dtype=np.uint16)
    pop_to[3] = 0
    pop_to[4] = 2
    h = guided.StackGuide("k", "s", trans, np.asarray([1, 0], dtype=np.uint8), pop_to)
    assert h.walk(0, b"p") == (1, (3,)) and h.walk(0, b"pq") == (0, ()) and h.matches(b"pq")
    for dead in (b"f", b"t", b"pr", b"q", b"ppq", b"pqq"):
        assert h.walk(0, dead) == (-1, ()), dead


# ---------------- compile_json_schema ----------------
def valid(sch, v, root=None) -> bool:
    """A hand-written validator of the supported subset (declared key order included)."""
    root = sch if root is None else root
    if sch is True or not [k for k in sch if k not in ("title", "description", "$defs", "definitions")]:
        return True
    if "$ref" in sch:
        _, where, name = sch["$ref"].split("/")
        return valid(root[where][name], v, root)
    if "enum" in sch or "const" in sch:
        return any(type(v) is type(e) and v == e for e in sch.get("enum", [sch.get("const")]))
    t = sch["type"]
    if t == "object":
        if not isinstance(v, dict):
            return False
        if "properties" not in sch:
            return True
        props = list(sch["properties"])
        return list(v) == [k for k in props if k in v] and all(k in v for k in sch.get("required", [])) \
            and all(valid(sch["properties"][k], v[k], root) for k in v)
    if t == "array":
        if not isinstance(v, list):
            return False
        if "items" not in sch:
            return True
        return sch.get("minItems", 0) <= len(v) <= sch.get("maxItems", 1 << 30) and all(valid(sch["items"], x, root) for x in v)
    if t == "string":
        return isinstance(v, str) and sch.get("minLength", 0) <= len(v) <= sch.get("maxLength", 1 << 30)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "boolean":
        return isinstance(v, bool)
    return v is None


BIG = {"type": "object", "title": "a request", "$defs": {"tag": {"enum": ["a", "b", 1, 1.5, True, None, "ab"]}},
       "properties": {"name": {"type": "string", "minLength": 1, "maxLength": 3, "description": "characters, not bytes"},
                      "n": {"type": "integer"}, "x": {"type": "number"}, "ok": {"type": "boolean"},
                      "tags": {"type": "array", "items": {"$ref": "#/$defs/tag"}, "minItems": 1, "maxItems": 3},
                      "nums": {"type": "array", "items": {"type": "integer"}},
                      "extra": {}, "obj": {"type": "object"}, "arr": {"type": "array"}, "nil": {"type": "null"},
                      "c": {"const": "only"}},
       "required": ["name", "ok"], "additionalProperties": False}
POOL = {"name": ["", "a", "abc", "abcd", "é€", "éé\U0001F600", "éé€x", 5, None], "n": [0, -12, 1.5, "1", True, 10 ** 20],
        "x": [0, -1.5, 2e-9, "x", None], "ok": [True, False, None, 0],
        "tags": [[], ["a"], ["ab", 1, None], ["a", "b", "a", "b"], ["c"], [1.5, True], [1.0], "a"],
        "nums": [[], [1], [1, -2, 3, 4, 5, 6], [1.5], [[1]]], "extra": [1, "s", None, {"q": [1, {"r": "}"}]}, [[], {}]],
        "obj": [{}, {"any": [1, 2]}, [], 1], "arr": [[], [1, {"a": []}], {}, "x"], "nil": [None, 0, False],
        "c": ["only", "onl", "only2", 1], "zzz": [1]}


def test_schema_guide_agrees_with_the_validator():
    g = guided.compile_json_schema(BIG)
    assert g.nstates <= guided.MAX_STATES and g.key == guided.compile_json_schema(json.dumps(BIG)).key
    rng = random.Random(3)
    order = list(BIG["properties"])
    seen = {True: 0, False: 0}
    for i in range(3000):
        keys = [k for k in order if rng.random() < 0.5 or (k in BIG["required"] and rng.random() < 0.9)]
        if rng.random() < 0.1:
            rng.shuffle(keys)
        if rng.random() < 0.05:
            keys.append("zzz")
        bias = 0.75 if i % 2 else 0.0     # half the draws mostly take the first (valid) candidates
        v = {k: (POOL[k][0 if k not in ("name", "tags") else 1] if rng.random() < bias else rng.choice(POOL[k])) for k in keys}
        want = valid(BIG, v)
        seen[want] += 1
        for seps in ((",", ":"), (", ", ": ")):
            data = json.dumps(v, separators=seps, ensure_ascii=False).encode()
            assert g.matches(data) == want, (data, want)
            if want:
                assert all(g.is_prefix(data[:n]) and not g.matches(data[:n]) for n in range(len(data)))
    assert seen[True] > 200 and seen[False] > 200
    # whitespace: one optional space after `:` and `,`, nothing else outside the free-form positions
    assert g.matches(b'{"name": "a", "ok": true, "extra": {"q" : [ 1 ,\n2 ]\t}}')
    for data in (b'{ "name":"a","ok":true}', b'{"name" :"a","ok":true}', b'{"name":  "a","ok":true}',
                 b'{"name":"a" ,"ok":true}', b'{"name":"a","ok":true }', b'{"name":"a","ok":true,"nums":[ 1]}'):
        assert not g.matches(data), data
    # top-level scalars and arrays; a finite schema is a finite language
    assert guided.compile_json_schema({"type": "integer"}).matches(b"-120") and not guided.compile_json_schema({"type": "integer"}).matches(b"01")
    assert guided.compile_json_schema({"type": "array", "items": {"type": "number"}, "minItems": 2}).matches(b"[1, 2.5e3,-0]")
    assert not guided.compile_json_schema({"type": "array", "items": {"type": "number"}, "minItems": 2}).matches(b"[1]")
    assert guided.compile_json_schema(True).matches(b'[{"a":1}]') and guided.compile_json_schema({}).matches(b'"s"')
    fin = guided.compile_json_schema({"type": "object", "properties": {"a": {"type": "boolean"}, "b": {"enum": ["x", "yz"]}},
                                      "required": ["a"]})
    assert not (fin.trans & guided.POP)[fin.trans != guided.DEAD].any() and not fin.trans[fin.walk(0, b'{"a":true}')[0]].min() < guided.DEAD


UNSUPPORTED = [
    ({"type": "string", "pattern": "a+"}, "pattern", "/pattern"),
    ({"type": "object", "properties": {"a": {"type": "string", "format": "date"}}}, "format", "/properties/a/format"),
    ({"anyOf": [{"type": "string"}]}, "anyOf", "/anyOf"),
    ({"type": "array", "items": {"oneOf": [{}]}}, "oneOf", "/items/oneOf"),
    ({"allOf": [{}]}, "allOf", "/allOf"),
    ({"not": {}}, "not", "/not"),
    ({"type": "object", "properties": {"a": {}}, "additionalProperties": True}, "additionalProperties", "/additionalProperties"),
    ({"type": "object", "additionalProperties": {"type": "string"}}, "additionalProperties", "/additionalProperties"),
    ({"type": "object", "patternProperties": {"a": {}}}, "patternProperties", "/patternProperties"),
    ({"type": ["string", "null"]}, "list of types", "/type"),
    ({"$ref": "#/$defs/n", "$defs": {"n": {"type": "array", "items": {"$ref": "#/$defs/n"}}}}, "recursive", "/$defs/n/items/$ref"),
    ({"enum": [1, [2]]}, "not a scalar", "/enum"),
    ({"type": "object", "properties": {"a/b": {"const": {"x": 1}}}}, "not a scalar", "/properties/a~1b/const"),
    ({"$ref": "http://example.com/s.json"}, "$ref", "/$ref"),
    ({"type": "string", "minimum": 3}, "minimum", "/minimum"),
]


@pytest.mark.parametrize("schema,names,pointer", UNSUPPORTED, ids=[u[1] + u[2].replace("/", "_") for u in UNSUPPORTED])
def test_unsupported_keywords_are_named_with_their_pointer(schema, names, pointer):
    with pytest.raises(ValueError) as e:
        guided.compile_json_schema(schema)
    assert names in str(e.value) and f" at {pointer} " in str(e.value) and str(e.value).startswith("guided_json:")


def test_schema_caps():
    with pytest.raises(ValueError, match=f"more than {guided.MAX_STATES} DFA states"):
        guided.compile_json_schema({"type": "string", "maxLength": 400})
    assert guided.compile_json_schema({"type": "string", "maxLength": 100}).nstates <= guided.MAX_STATES
    with pytest.raises(ValueError, match="larger than 16384 bytes"):
        guided.compile_json_schema({"type": "string", "description": "x" * 16384})
    with pytest.raises(ValueError, match="larger than 16384 bytes"):
        guided.compile_json_schema(json.dumps({"type": "string", "description": "x" * 16384}))
    free = lambda n: {"type": "object", "properties": {"p%d" % i: {} for i in range(n)}}   # noqa: E731
    eleven = guided.compile_json_schema(free(11))
    assert eleven.matches(b'{"p0":[1],"p10":{"a":[]}}') and (eleven.pop_to[1:15] < eleven.nstates).sum() == 13
    with pytest.raises(ValueError, match=r"free-form position at /properties/p\d+ .* at most 11"):
        guided.compile_json_schema(free(12))
    for bad in ("[1]", "not json", 5, None, [1]):
        with pytest.raises(ValueError, match="guided_json"):
            guided.compile_json_schema(bad)


# ---------------- the mask definition ----------------
def test_case_preconditions():
    jc.check_preconditions()


@pytest.mark.parametrize("case", jc.CASES, ids=lambda c: c.id)
def test_reference_mask_is_the_literal_definition(case):
    want = jc.literal(case)
    got = jc.run_ops(case, "cpu")
    assert len(got) == 5 and all(g.dtype == torch.int32 for g in got) and got[0].shape == want[0].shape
    for name, g, w in zip(("bits", "idx", "state_after", "depth_after", "stack_after"), got, want):
        assert np.array_equal(g.numpy().view(w.dtype), w), name


def test_dfa_rows_of_the_stack_op_equal_guide_mask():
    """The regex / choice cases of guided_cases through guide_mask_stack with kind 0: the old semantics exactly."""
    from ai_agent_kubectl_amd import ops
    for c in gc.CASES[:12]:
        def dev(a, view=None):
            return None if a is None else torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view)))
        R, G = c.rows, c.trans.shape[0]
        rng = np.random.RandomState(R)
        pop = torch.from_numpy(rng.randint(0, 4, size=(G, 16)).astype(np.int16))
        got = ops.guide_mask_stack(gc.token_table(c.V), dev(c.trans, np.int16), dev(c.accept), pop, dev(c.row_base),
                                   dev(c.row_nstates), dev(c.row_state), torch.zeros(R, dtype=torch.int32),
                                   torch.from_numpy(rng.randint(-2, 70, size=R).astype(np.int32)),
                                   torch.from_numpy(rng.randint(0, 2 ** 31 - 1, size=(R, 8)).astype(np.int32)),
                                   dev(c.pend_src), dev(c.tokens), dev(c.base_bits, np.int32), dev(c.base_idx))
        want = gc.literal(c)
        assert all(np.array_equal(g.numpy().view(w.dtype), w) for g, w in zip(got[:3], want))
        assert not got[3].any() and not got[4].any()


# ---------------- host bookkeeping ----------------
class _Tok:
    eos_ids = (2,)
    id_to_bytes = [b'{"a":', b"[", None, b"]", b"1", b"}", b"x", b"[[", b"]]}"]
    vocab_size = 9

    def is_eos(self, t):
        return t in self.eos_ids

    def token_bytes(self, t):
        return self.id_to_bytes[t] or b""

    def decode(self, ids):
        return b"".join(self.token_bytes(t) for t in ids).decode()


def test_guide_state_holds_its_stack_across_placeholders_and_a_recompute(jobj):
    tok = _Tok()
    s = Sequence(prompt_ids=[6, 6], params=SamplingParams(guide=jobj), forced_prefix=[0])
    st = guided.state_of(s, tok)
    assert st.counted == 1 and (st.state, st.stack) == jobj.walk(0, b'{"a":') and st.stack == (guided.SYM_TOP,)
    s.output_ids.append(PLACEHOLDER)             # a step in flight: not walked
    assert guided.state_of(s, tok).counted == 1 and st.stack == (guided.SYM_TOP,)
    s.output_ids[-1] = 7                          # settled: "[["
    s.output_ids.append(PLACEHOLDER)
    assert guided.state_of(s, tok).counted == 2 and st.stack == (guided.SYM_TOP, guided.SYM_OBJ, guided.SYM_ARR)
    s.output_ids[-1] = 2                          # EOS moves neither the state nor the stack
    assert guided.state_of(s, tok).counted == 3 and len(st.stack) == 3
    s.num_computed, s.block_table = 0, []         # a recompute preemption drops the KV, not the outputs
    s.output_ids.append(8)                        # "]]}": pops all three
    assert guided.state_of(s, tok) is st and st.counted == 4 and st.stack == () and jobj.accept[st.state]
    s.output_ids.append(5)                        # "}" after the end: dead, and it stays dead
    s.output_ids.append(1)
    assert guided.state_of(s, tok).state == -1 and st.stack == ()


def test_pack_guide_stacks_layout_and_the_table_uploads_pop_to(jobj):
    tok = _Tok()
    rx = guided.compile_regex("zz")
    t = guided.GuideTable(states=256, device="cpu")
    assert t.arena_pop.shape == (256, 16) and t.arena_pop.dtype == torch.int16 and bool((t.arena_pop == -1).all())
    seqs = [Sequence(prompt_ids=[6], params=SamplingParams()), Sequence(prompt_ids=[6], params=SamplingParams(guide=rx)),
            Sequence(prompt_ids=[6], params=SamplingParams(guide=jobj)), Sequence(prompt_ids=[6], params=SamplingParams(guide=jobj))]
    seqs[1].guide_ref = t.acquire(rx)
    seqs[2].guide_ref = seqs[3].guide_ref = t.acquire(jobj)
    assert (seqs[1].guide_ref.kind, seqs[2].guide_ref.kind) == (0, 1)
    deep = b'{"a":' + b"[" * 9
    seqs[3].output_ids += [0] + [1] * 9 + [PLACEHOLDER]
    img = guided.pack_guide_stacks(seqs, 5, tok)
    assert img.dtype == np.int32 and img.shape == (50,)
    assert img[0:5].tolist() == [0, 0, 1, 1, 0] and img[5:10].tolist() == [0, 0, 0, 10, 0]
    words = img[10:].view(np.uint32).reshape(5, 8)
    assert not words[[0, 1, 2, 4]].any()
    want = jobj.walk(0, deep, (), per_token=False)[1]
    assert want == (1, 2) + (3,) * 8 and words[3].tolist() == [0x33333321, 0x33] + [0] * 6
    assert np.array_equal(guided.pack_stack(want), words[3])
    # pack_guides is unchanged: the 4 * rows image, also for a stack sequence
    old = guided.pack_guides(seqs, 5, [-1, -1, -1, 3, -1], tok)
    base = seqs[3].guide_ref.base
    assert old.shape == (20,) and old[0:5].tolist() == [-1, 0, base, base, -1] and old[15:].tolist() == [-1, -1, -1, 3, -1]
    assert old[5:10].tolist() == [0, rx.nstates, jobj.nstates, jobj.nstates, 0] and old[13] == jobj.walk(0, deep, (), per_token=False)[0]
    t.flush()
    assert np.array_equal(t.arena_pop[base].numpy().view(np.uint16), jobj.pop_to)
    assert bool((t.arena_pop[0] == -1).all()) and bool((t.arena_pop[base + 1:] == -1).all())   # DFA guides and other rows: dead
    assert np.array_equal(t.trans[base:base + jobj.nstates].numpy().view(np.uint16), jobj.trans)


def test_validate_a_stack_guide(jobj):
    tok = _Tok()
    with pytest.raises(ValueError, match=r"guided_json / response_format are not supported with tensor parallelism \(TP > 1\)"):
        guided.validate(SamplingParams(guide=jobj), tok, 2)
    with pytest.raises(ValueError, match="this tokenizer cannot spell the pattern"):
        guided.validate(SamplingParams(guide=jobj), tok, 1)
    # pops are continuations: a guide whose only way on from a state is a pop validates when a token spells the byte
    trans = np.full((2, 256), guided.DEAD, dtype=np.uint16)
    trans[0, ord("[")] = 1 | (guided.SYM_TOP << 11)
    trans[1, ord("]")] = guided.POP
    pop_to = np.full(16, guided.DEAD, dtype=np.uint16)
    pop_to[guided.SYM_TOP] = 0
    g = guided.StackGuide("k", "s", trans, np.asarray([1, 0], dtype=np.uint8), pop_to)
    guided.validate(SamplingParams(guide=g), tok, 1)
    guided.validate(SamplingParams(guide=g), tok, 1, forced_prefix=[1, 3, 1, 3])
    with pytest.raises(ValueError, match="forced prefix"):
        guided.validate(SamplingParams(guide=g), tok, 1, forced_prefix=[1, 3, 3])


# ---------------- engine (tiny-llama) ----------------
@pytest.fixture(scope="module")
def tiny():
    from ai_agent_kubectl_amd.engine.builder import EngineOptions, build_engine
    from ai_agent_kubectl_amd.llm.engine_backend import EngineLLM
    eng = build_engine(EngineOptions(model="tiny-llama", device="cpu", max_batch=8, graph_buckets=(1, 2, 4, 8),
                                     kv_cache_tokens=8192, max_model_len=512))
    return eng, EngineLLM(eng, max_new_tokens=8)


Q = "list pods in prod"
PAT = r"kubectl (get|describe) (pods|nodes|svc) -n [a-z0-9-]{1,6}"
FINITE = {"type": "object", "properties": {"ok": {"type": "boolean"}, "kind": {"enum": ["pod", "node", 7]},
                                           "flags": {"type": "array", "items": {"type": "boolean"}, "maxItems": 2}},
          "required": ["ok", "kind"]}


def _text(eng, seq):
    tok = eng.tokenizer
    return tok.decode([t for t in seq.output_ids if not tok.is_eos(t)])


def _alone(eng, be, query, params, forced=False):
    eng.bm.reset_prefix_cache()
    return eng.generate_blocking([be.prompt_ids(query)], params, forced_prefix=be._forced if forced else None)[0]


def _legal_json_object(g, seq, text):
    if seq.finish_reason == "stop":
        return isinstance(json.loads(text), dict)
    return seq.finish_reason == "length" and g.is_prefix(text.encode())


def test_json_object_parses_or_is_a_prefix(tiny, jobj):
    eng, be = tiny
    st = eng.runner.stats
    j0, g0 = st["json_steps"], st["guided_steps"]
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=24, safe_decode=False, guide=jobj))
    assert _legal_json_object(jobj, s, _text(eng, s)), _text(eng, s)
    assert st["json_steps"] == j0 + len(s.output_ids) and st["guided_steps"] == g0 + len(s.output_ids)
    outcomes = set()
    for seed in range(1, 7):
        p = SamplingParams(max_new_tokens=24, safe_decode=False, guide=jobj, temperature=1.0, seed=seed)
        s = _alone(eng, be, Q, p)
        assert _legal_json_object(jobj, s, _text(eng, s)), _text(eng, s)
        outcomes.add(s.finish_reason)
        if seed == 1:
            assert _alone(eng, be, Q, p).output_ids == s.output_ids
    assert s.guide_ref is None and all(p.refs == 0 for p in eng.runner.guide_table.placed.values())


def test_a_finite_schema_always_stops_and_validates(tiny):
    eng, be = tiny
    f = guided.compile_json_schema(FINITE)
    texts = set()
    for kw in (dict(), dict(temperature=1.0, seed=1), dict(temperature=1.5, seed=2), dict(temperature=2.0, seed=3)):
        s = _alone(eng, be, Q, SamplingParams(max_new_tokens=64, safe_decode=False, guide=f, **kw))
        assert s.finish_reason == "stop", _text(eng, s)
        v = json.loads(_text(eng, s))
        assert valid(FINITE, v) and f.matches(_text(eng, s).encode()), v
        texts.add(_text(eng, s))
    assert len(texts) > 1


def test_logprobs_of_a_json_request_stay_inside_the_guide(tiny, jobj):
    eng, be = tiny
    tok = eng.tokenizer
    s = _alone(eng, be, Q, SamplingParams(max_new_tokens=16, safe_decode=False, guide=jobj, logprobs=20))
    assert len(s.logprobs) == len(s.generated)
    state, stack = 0, ()
    for t, rec in zip(s.generated, s.logprobs):
        live = [i for i in rec.top_ids if i >= 0]
        for i in live:
            if tok.is_eos(i):
                assert jobj.accept[state]
            else:
                assert tok.token_bytes(i) and jobj.walk(state, tok.token_bytes(i), stack)[0] >= 0, (state, tok.token_bytes(i))
        assert t in live and np.isfinite(rec.logprob) and rec.logprob <= 0.0
        if not tok.is_eos(t):
            state, stack = jobj.walk(state, tok.token_bytes(t), stack)


OTHERS = [("get svc -A", dict(max_new_tokens=3, ignore_eos=True)),
          ("top nodes", dict(max_new_tokens=6, ignore_eos=True, frequency_penalty=2.0, logprobs=2)),
          ("get nodes -o wide", dict(max_new_tokens=7, ignore_eos=True))]


@pytest.mark.parametrize("lookahead", [True, False], ids=["lookahead", "no-lookahead"])
def test_same_bytes_alone_and_in_mixed_company(tiny, jobj, lookahead):
    eng, be = tiny
    f, rx = guided.compile_json_schema(FINITE), guided.compile_regex(PAT)
    pj = dict(max_new_tokens=20, safe_decode=False, guide=jobj, temperature=0.9, seed=11)
    pf = dict(max_new_tokens=64, safe_decode=False, guide=f)
    pr = dict(max_new_tokens=48, safe_decode=False, guide=rx)
    want_j, want_f, want_r = (_alone(eng, be, Q, SamplingParams(**p)) for p in (pj, pf, pr))
    alone = [_alone(eng, be, q, SamplingParams(**kw), forced=True) for q, kw in OTHERS]
    # chained behind a token still on the device: the kernel completes state and stack from d_out
    eng.bm.reset_prefix_cache()
    assert gc.chain_async(eng, Sequence(prompt_ids=be.prompt_ids(Q), params=SamplingParams(**pj))) == want_j.output_ids
    eng.bm.reset_prefix_cache()
    assert gc.chain_async(eng, Sequence(prompt_ids=be.prompt_ids(Q), params=SamplingParams(**pf))) == want_f.output_ids
    # one prompt admitted per step: every step after the first is a mixed decode + prefill step
    eng.bm.reset_prefix_cache()
    outs = engine_helpers.run_staggered(eng, [be.prompt_ids(Q), be.prompt_ids(Q)], SamplingParams(**pf), [])
    assert outs == [want_f.output_ids] * 2 and engine_helpers.run_staggered.mixed > 0
    # the threaded engine beside a regex-guided request and plain, penalised and logprobs requests
    eng.bm.reset_prefix_cache()
    done, ev = [], threading.Event()

    def cb(seq):
        done.append(seq)
        if len(done) == len(OTHERS) + 3:
            ev.set()

    n0, sch = eng.lookahead_steps, eng.scheduler
    saved = sch.max_batched_tokens, sch.min_chunk, eng.lookahead
    sch.max_batched_tokens, sch.min_chunk, eng.lookahead = 40, 4, lookahead
    j0 = eng.runner.stats["json_steps"]
    eng.start()
    try:
        first = eng.submit(be.prompt_ids(OTHERS[0][0]), SamplingParams(**OTHERS[0][1]), cb, forced_prefix=be._forced)
        a = eng.submit(be.prompt_ids(Q), SamplingParams(**pj), cb)
        b = eng.submit(be.prompt_ids(Q), SamplingParams(**pf), cb)
        c = eng.submit(be.prompt_ids(Q), SamplingParams(**pr), cb)
        rest = [eng.submit(be.prompt_ids(q), SamplingParams(**kw), cb, forced_prefix=be._forced) for q, kw in OTHERS[1:]]
        assert ev.wait(120)
    finally:
        eng.shutdown()
        sch.max_batched_tokens, sch.min_chunk, eng.lookahead = saved
    assert eng.healthy and (eng.lookahead_steps > n0) == lookahead
    assert a.output_ids == want_j.output_ids and b.output_ids == want_f.output_ids and c.output_ids == want_r.output_ids
    for got, ref_run in zip([first] + rest, alone):   # and nobody else's bytes moved
        assert got.output_ids == ref_run.output_ids
    assert eng.runner.stats["json_steps"] > j0
    assert all(p.refs == 0 for p in eng.runner.guide_table.placed.values())


def test_plain_and_regex_only_steps_stage_no_stack_image(tiny):
    eng, be = tiny
    before = eng.runner.stats["json_steps"]
    staged = []
    orig = eng.runner._stage_guide_stacks
    eng.runner._stage_guide_stacks = lambda *a, **k: staged.append(1) or orig(*a, **k)
    try:
        _alone(eng, be, Q, SamplingParams(max_new_tokens=4, ignore_eos=True), forced=True)
        _alone(eng, be, Q, SamplingParams(max_new_tokens=4, ignore_eos=True, temperature=0.8, seed=1), forced=True)
        g0 = eng.runner.stats["guided_steps"]
        s = _alone(eng, be, Q, SamplingParams(max_new_tokens=48, safe_decode=False, guide=guided.compile_regex(PAT)))
        assert re.fullmatch(PAT, _text(eng, s)) and eng.runner.stats["guided_steps"] == g0 + len(s.output_ids)
    finally:
        eng.runner._stage_guide_stacks = orig
    assert not staged and eng.runner.stats["json_steps"] == before


# ---------------- HTTP ----------------
def _client(be):
    from fastapi.testclient import TestClient
    from ai_agent_kubectl_amd.api import create_app
    from ai_agent_kubectl_amd.config import Settings
    return TestClient(create_app(Settings(RATE_LIMIT="1000/minute", MODEL="tiny-llama"), backend=be))


BODY = {"model": "tiny-llama", "messages": [{"role": "user", "content": "list pods"}], "max_tokens": 64}
URL = "/v1/chat/completions"
SMALL = {"type": "object", "properties": {"ok": {"type": "boolean"}, "kind": {"enum": ["pod", "node"]}}, "required": ["ok", "kind"]}


def test_http_fields(tiny):
    eng, be = tiny
    st = eng.runner.stats
    with _client(be) as c:
        before, cached = st["guided_steps"], len(be._guides)
        plain = c.post(URL, json=BODY)
        text = c.post(URL, json=dict(BODY, response_format={"type": "text"}))
        assert plain.status_code == text.status_code == 200 and st["guided_steps"] == before   # a no-op
        assert text.json()["choices"][0]["message"] == plain.json()["choices"][0]["message"]
        r = c.post(URL, json=dict(BODY, max_tokens=24, response_format={"type": "json_object"}, temperature=1.0, seed=2))
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        if ch["finish_reason"] == "stop":
            assert isinstance(json.loads(ch["message"]["content"]), dict)
        else:
            assert guided.compile_json_object().is_prefix(ch["message"]["content"].encode())
        assert st["json_steps"] > 0 and set(ch) == {"index", "message", "finish_reason"}
        forms = [dict(response_format={"type": "json_schema", "json_schema": {"name": "x", "schema": SMALL, "strict": True}}),
                 dict(guided_json=SMALL), dict(guided_json=json.dumps(SMALL))]
        for kw in forms:
            r = c.post(URL, json=dict(BODY, **kw))
            assert r.status_code == 200, r.text
            ch = r.json()["choices"][0]
            assert ch["finish_reason"] == "stop" and valid(SMALL, json.loads(ch["message"]["content"])), ch
        assert len(be._guides) == cached + 2   # json_object and one schema source, compiled once
        # the other fields work beside it
        r = c.post(URL, json=dict(BODY, guided_json=SMALL, temperature=0.8, seed=4, logprobs=True, top_logprobs=3,
                                  frequency_penalty=0.5, logit_bias={"1000": 5}))
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        assert valid(SMALL, json.loads(ch["message"]["content"]))
        assert "".join(e["token"] for e in ch["logprobs"]["content"]) == ch["message"]["content"]
        cut = c.post(URL, json=dict(BODY, guided_json=SMALL, max_tokens=2)).json()["choices"][0]
        assert cut["finish_reason"] == "length" and guided.compile_json_schema(SMALL).is_prefix(cut["message"]["content"].encode())


def test_http_validation(tiny):
    eng, be = tiny
    js = lambda schema: {"type": "json_schema", "json_schema": {"name": "x", "schema": schema}}   # noqa: E731
    huge = {"type": "string", "description": "x" * 16384}
    with _client(be) as c:
        bad = [dict(response_format={"type": "yaml"}), dict(response_format={}), dict(response_format="json_object"),
               dict(response_format={"type": "json_schema"}), dict(response_format={"type": "json_schema", "json_schema": {"name": "x"}}),
               dict(response_format=js([1])), dict(response_format=js("string")), dict(response_format=js(huge)),
               dict(guided_json=huge), dict(guided_json=json.dumps(huge)), dict(guided_json="[1]"), dict(guided_json="{"),
               dict(guided_json=5), dict(guided_json=[1]),
               dict(response_format={"type": "json_object"}, guided_json=SMALL),
               dict(response_format={"type": "json_object"}, guided_regex="a+"),
               dict(response_format=js(SMALL), guided_choice=["a"]), dict(guided_json=SMALL, guided_regex="a+"),
               dict(guided_json=SMALL, guided_choice=["a"])]
        for kw in bad:
            assert c.post(URL, json=dict(BODY, **kw)).status_code == 422, kw
        assert c.post(URL, json=dict(BODY, response_format={"type": "text"}, guided_regex="a+", max_tokens=2)).status_code == 200
        for schema, names in (({"type": "string", "pattern": "a"}, "'pattern' at /pattern"),
                              ({"anyOf": [{}]}, "'anyOf' at /anyOf"),
                              ({"type": "string", "maxLength": 400}, "DFA states"),
                              ({"type": "object", "properties": {"p%d" % i: {} for i in range(12)}}, "free-form position")):
            for kw in (dict(guided_json=schema), dict(response_format=js(schema))):
                r = c.post(URL, json=dict(BODY, **kw))
                assert r.status_code == 400 and names in r.text, (kw, r.text)
        # a tokenizer without the single-byte tokens the guide needs
        have = guided.single_byte_tokens(eng.tokenizer)
        eng.tokenizer._guided_single_bytes = np.zeros(256, dtype=bool)
        try:
            r = c.post(URL, json=dict(BODY, response_format={"type": "json_object"}))
            assert r.status_code == 400 and "cannot spell the pattern" in r.text
        finally:
            eng.tokenizer._guided_single_bytes = have
        # a guide table with no room
        table = eng.runner.guides()
        eng.runner.guide_table = guided.GuideTable(states=16, device="cpu")
        try:
            r = c.post(URL, json=dict(BODY, response_format={"type": "json_object"}))
            assert r.status_code == 400 and "guide table is full" in r.text
        finally:
            eng.runner.guide_table = table
        # a tensor-parallel engine refuses before anything runs
        eng.runner.tp_size = 2
        try:
            for kw in (dict(response_format={"type": "json_object"}), dict(response_format=js(SMALL)), dict(guided_json=SMALL)):
                r = c.post(URL, json=dict(BODY, **kw))
                assert r.status_code == 400 and "TP > 1" in r.text and "response_format" in r.text, kw
            assert c.post(URL, json=dict(BODY, response_format={"type": "text"})).status_code == 200
        finally:
            eng.runner.tp_size = 1
