"""`LLM_BACKEND=engine`: the on-node MI355X inference engine behind the reference's chain call.

`generate(query)` does what `chain.ainvoke({"query": q})` did (`/root/reference/app.py:184`):
PromptTemplate.format (prompt.py) -> single user turn in the model's chat template -> greedy decode
(temperature 0) -> text for `KubectlOutputParser` semantics (safety.parse_llm_output).

Tokenisation keeps the instruction prefix as a separately encoded, cached token run so that every
request's prompt starts with identical token ids and the engine's prefix cache shares its KV blocks.
Cancellation (the service's `LLM_TIMEOUT` -> 504) aborts the sequence and frees its blocks.
"""
from __future__ import annotations

import asyncio
import collections
import concurrent.futures
import json
import logging
import threading
from typing import List, Optional

from ..engine import guided
from ..engine.safe_decode import forced_prefix
from ..engine.sequence import SamplingParams
from ..engine.streaming import StreamDecoder
from ..prompt import PROMPT_PREFIX, PROMPT_SUFFIX
from .base import LLMBackend, LLMUnavailableError

logger = logging.getLogger("app.engine")


class EngineLLM(LLMBackend):
    name = "engine"

    def __init__(self, engine, max_new_tokens: int = 24, ignore_eos: bool = False, safe_decode: bool = True):
        self.engine = engine
        self.tok = engine.tokenizer
        self.params = SamplingParams(max_new_tokens=max_new_tokens, ignore_eos=ignore_eos, safe_decode=safe_decode)
        before, after = self.tok.chat_prefix_suffix()
        self._prefix_ids: List[int] = before + self.tok.encode(PROMPT_PREFIX)
        self._after_ids: List[int] = after
        self._forced = forced_prefix(self.tok) if safe_decode else []
        self._started = False
        # compiled guides of guided_regex / guided_choice requests, by source (LRU, GUIDE_CACHE entries)
        self._guides: "collections.OrderedDict" = collections.OrderedDict()
        self._guides_lock = threading.Lock()
        self._compiling: dict = {}   # source -> Future of a compilation in progress

    @classmethod
    def from_settings(cls, settings, metrics=None) -> "EngineLLM":
        from ..engine.builder import EngineOptions, build_engine
        from ..models.lora import kubectl_slot

        opts = EngineOptions.from_settings(settings)
        comm = None
        if settings.TP > 1:
            from ..parallel.launch import init_tp

            comm, rank = init_tp(settings.TP)
            opts.tp_rank = rank
            opts.device = f"cuda:{rank}" if opts.device == "cuda" else opts.device
        eng = build_engine(opts, comm=comm, metrics=metrics)
        if opts.use_graphs and opts.device.startswith("cuda"):
            eng.runner.capture_graphs()
        llm = cls(eng, max_new_tokens=settings.MAX_NEW_TOKENS, ignore_eos=settings.IGNORE_EOS,
                  safe_decode=settings.SAFE_DECODE)
        llm.use_kubectl_adapter(kubectl_slot(settings))
        return llm

    def use_kubectl_adapter(self, slot: Optional[int]) -> None:
        """LORA_KUBECTL: /kubectl-command generations (`generate`) run on this adapter slot (None: the base model)."""
        if slot is not None and not 0 <= slot < len(self.engine.lora_names):
            raise ValueError(f"LORA_KUBECTL: slot {slot} is outside the engine's {len(self.engine.lora_names)} adapters")
        self.params.adapter = slot

    def prompt_ids(self, query: str) -> List[int]:
        return self._prefix_ids + self.tok.encode(query + PROMPT_SUFFIX) + self._after_ids

    async def start(self) -> None:
        if not self._started:
            from ..utils.runtime import tune_gc
            tune_gc()
            self.engine.start()
            self._started = True

    async def close(self) -> None:
        if self._started:
            self.engine.shutdown()
            self._started = False

    def healthy(self) -> bool:
        return self.engine.healthy

    def attach_metrics(self, metrics) -> None:
        if metrics is not None and getattr(self.engine, "metrics", None) is None:
            self.engine.metrics = metrics

    async def generate(self, query: str) -> str:
        if not self._started:
            await self.start()
        if not self.engine.healthy:
            raise LLMUnavailableError(f"engine unhealthy: {self.engine.last_error}")
        loop = asyncio.get_running_loop()
        fut: asyncio.Future = loop.create_future()

        def done(seq):
            loop.call_soon_threadsafe(_resolve, fut, seq)

        seq = self.engine.submit(self.prompt_ids(query), self.params, done, forced_prefix=self._forced)
        try:
            seq = await fut
        except asyncio.CancelledError:
            self.engine.abort(seq)
            raise
        if seq.error is not None:
            if seq.finish_reason == "error":
                raise LLMUnavailableError(str(seq.error))
            raise RuntimeError(str(seq.error))
        ids = [t for t in seq.output_ids if not self.tok.is_eos(t)]
        return self.tok.decode(ids)

    def stats(self):
        return dict(self.engine.runner.stats)

    # ---- OpenAI-compatible chat (api/openai_compat.py) ----------------------------------------
    def chat_ids(self, messages) -> List[int]:
        """Multi-turn chat template of the model family (Llama-3 header tokens / Llama-2 [INST])."""
        tok = self.tok
        if tok.family == "llama3":
            s = tok.specials
            ids = [s["<|begin_of_text|>"]]
            for m in messages:
                ids += [s["<|start_header_id|>"]] + tok.encode(m["role"]) + [s["<|end_header_id|>"]]
                ids += tok.encode("\n\n" + m["content"]) + [s["<|eot_id|>"]]
            ids += [s["<|start_header_id|>"]] + tok.encode("assistant") + [s["<|end_header_id|>"]] + tok.encode("\n\n")
            return ids
        text = "".join(f"[INST] {m['content']} [/INST]" if m["role"] != "assistant" else f" {m['content']} "
                       for m in messages)
        return [tok.bos_id] + tok.encode(text)

    async def generate_chat(self, messages, max_tokens: int = 64, safe: bool = False, temperature: float = 0.0,
                            top_p: float = 1.0, top_k: int = 0, seed: Optional[int] = None, with_stop: bool = False,
                            **penalties):
        """Returns (text, finish_reason, prompt_tokens, completion_tokens).  temperature 0 (the default)
        decodes greedily; above it the engine samples (top_k / top_p cuts, `seed` makes it repeatable).
        penalties: presence_penalty, frequency_penalty, repetition_penalty, logit_bias ({token id: bias}),
        applied to the logits before the token is chosen, also at temperature 0 (SamplingParams); and
        guided_regex or guided_choice: the completion then matches the pattern / is one of the choices when it
        ends with "stop", and is a prefix of a match when max_tokens cuts it (engine/guided.py); json_object=True
        (any JSON object) or guided_json (a JSON Schema of the supported subset, dict or string): JSON mode;
        stop (1..4 byte strings of 1..64 bytes): the text ends before the first of them that occurs, with "stop";
        with_stop=True appends the index of the stop string that matched (None: EOS or length) to the result.
        Raises ValueError for a request the engine cannot serve (temperature > 0, penalties or a guide under
        TP > 1, a logit_bias id outside the vocabulary, a pattern outside the dialect or that the tokenizer
        cannot spell, a full guide table)."""
        seq, n_in = await self._chat(messages, max_tokens, safe, temperature, top_p, top_k, seed, None, **penalties)
        res = assemble_chat(self.tok, seq.output_ids, seq.n_forced, None, seq.finish_reason, seq.stop_cut, n_in)[:4]
        return res + (seq.stop_match,) if with_stop else res

    async def generate_chat_logprobs(self, messages, top_logprobs: int = 0, max_tokens: int = 64, safe: bool = False,
                                     temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0,
                                     seed: Optional[int] = None, with_stop: bool = False, **penalties):
        """generate_chat with per-token log-probabilities: returns its four values and OpenAI's
        `logprobs.content` list, one {"token", "logprob", "bytes", "top_logprobs": [{"token", "logprob",
        "bytes"}, ...]} per model-generated token that makes up the text (the stripped EOS, a
        jump-forward prefix and a token that starts at or past a stop cut have none), with `top_logprobs`
        (0..20) alternatives each.  The values are
        the model's distribution under the token mask before temperature / top_k / top_p and before the
        penalties and logit_bias (ops.token_logprobs): a token's logprob is its raw one.
        Raises ValueError under TP > 1."""
        seq, n_in = await self._chat(messages, max_tokens, safe, temperature, top_p, top_k, seed, int(top_logprobs),
                                     **penalties)
        res = assemble_chat(self.tok, seq.output_ids, seq.n_forced, seq.logprobs, seq.finish_reason, seq.stop_cut, n_in)
        return res + (seq.stop_match,) if with_stop else res

    async def stream_chat(self, messages, top_logprobs: Optional[int] = None, max_tokens: int = 64, safe: bool = False,
                          temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0, seed: Optional[int] = None,
                          **penalties):
        """generate_chat (top_logprobs None) / generate_chat_logprobs as an async generator of events: first
        {"prompt_tokens"}, then {"text", "logprobs": [entries] | None} at most once per engine step and only when
        something is released (engine/streaming.py StreamDecoder), then {"finish_reason", "stop_reason",
        "completion_tokens"} (stop_reason: the index of the stop string that matched, or None).  The released texts
        join to generate_chat's text and the entries to generate_chat_logprobs' list.  A request the engine cannot
        serve raises ValueError before the first event.  Closing the generator, or cancelling its consumer, aborts
        the sequence: its KV blocks and its guide range are free again."""
        loop = asyncio.get_running_loop()
        events: asyncio.Queue = asyncio.Queue()
        logprobs = None if top_logprobs is None else int(top_logprobs)

        def on_tokens(sq, first):   # engine thread: hand the ids and records over, nothing else
            loop.call_soon_threadsafe(events.put_nowait, (sq.output_ids[first:], sq.logprobs[first - sq.n_forced:]
                                                          if logprobs is not None else None))

        seq, n_in = await self._submit_chat(messages, lambda sq: loop.call_soon_threadsafe(events.put_nowait, sq),
                                            on_tokens, max_tokens, safe, temperature, top_p, top_k, seed, logprobs,
                                            **penalties)
        try:
            yield {"prompt_tokens": n_in}
            out = ChatStream(self.tok, seq.params.stop, logprobs is not None, seq.output_ids[:seq.n_forced])
            while True:
                ev = await events.get()
                if ev is seq:
                    break
                ev = out.push(*ev, emit=not seq.finished)
                if ev is not None:
                    yield ev
            if seq.error is not None:
                raise LLMUnavailableError(str(seq.error))
            for ev in out.finish(seq.finish_reason, len(seq.output_ids)):
                yield ev
        finally:
            if not seq.finished:
                self.engine.abort(seq)

    GUIDE_CACHE = 64

    def compile_guide(self, guided_regex: Optional[str] = None, guided_choice: Optional[List[str]] = None,
                      guided_json=None, json_object: bool = False):
        """The compiled guide of a request (engine/guided.py), from an LRU of the last GUIDE_CACHE sources; the
        first guided request also builds the engine's token table and guide arena here.  Host work that the
        compiler's caps and work budget keep to a fraction of a second (the token table: once per engine):
        `_chat` runs it on a worker thread, off the event loop and off the engine's loop.  Requests that arrive
        with a source that is being compiled wait for that compilation.  Raises ValueError for a pattern
        outside the dialect or past a cap."""
        if (guided_regex is not None) + (guided_choice is not None) + (guided_json is not None) + bool(json_object) > 1:
            raise ValueError("guided_regex, guided_choice, guided_json and response_format cannot be combined")
        if guided_json is not None and not isinstance(guided_json, str):
            try:
                guided_json = json.dumps(guided_json, ensure_ascii=False, allow_nan=False)   # key order kept: it is the members' order
            except (TypeError, ValueError) as e:
                raise ValueError(f"guided_json: the schema is not JSON ({e})") from None
        key = (("regex", guided_regex) if guided_regex is not None else ("json_object",) if json_object
               else ("json", guided_json) if guided_json is not None else ("choice", tuple(guided_choice)))
        with self._guides_lock:
            g = self._guides.get(key)
            if g is not None:
                self._guides.move_to_end(key)
                return g
            fut = self._compiling.get(key)
            mine = fut is None
            if mine:
                fut = self._compiling[key] = concurrent.futures.Future()
        if not mine:
            return fut.result()
        try:
            g = (guided.compile_regex(guided_regex) if guided_regex is not None
                 else guided.compile_json_object() if json_object
                 else guided.compile_json_schema(guided_json) if guided_json is not None
                 else guided.compile_choice(list(guided_choice)))
            if self.engine.runner.tp_size == 1:   # a TP engine refuses the request at submit: nothing to build
                self.engine.runner.guides()
        except BaseException as e:
            with self._guides_lock:
                del self._compiling[key]
            fut.set_exception(e)
            raise
        with self._guides_lock:
            self._guides[key] = g
            self._guides.move_to_end(key)
            while len(self._guides) > self.GUIDE_CACHE:
                self._guides.popitem(last=False)
            del self._compiling[key]
        fut.set_result(g)
        return g

    def chat_params(self, max_tokens, safe, temperature, top_p, top_k, seed, logprobs, guide=None,
                    presence_penalty: float = 0.0, frequency_penalty: float = 0.0, repetition_penalty: float = 1.0,
                    logit_bias=None, stop=None, adapter: Optional[int] = None) -> SamplingParams:
        return SamplingParams(max_new_tokens=max_tokens, ignore_eos=False, safe_decode=safe,
                              temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=seed,
                              logprobs=logprobs, presence_penalty=float(presence_penalty),
                              frequency_penalty=float(frequency_penalty),
                              repetition_penalty=float(repetition_penalty),
                              logit_bias={int(t): float(b) for t, b in logit_bias.items()} if logit_bias else None,
                              guide=guide, stop=[bytes(x) for x in stop] if stop else None, adapter=adapter)

    def submit_chat(self, messages, done, on_tokens, max_tokens, safe, temperature, top_p, top_k, seed, logprobs,
                    guided_regex: Optional[str] = None, guided_choice: Optional[List[str]] = None,
                    guided_json=None, json_object: bool = False, guide=None, **fields):
        """Compile the request's guide unless the caller did (host work: off the event loop and off the engine's
        thread) and submit it -> (sequence, prompt tokens).  `done(seq)` and `on_tokens(seq, first)` run on the
        engine thread."""
        if guide is None and (guided_regex is not None or guided_choice is not None or guided_json is not None
                              or json_object):
            guide = self.compile_guide(guided_regex, guided_choice, guided_json, json_object)
        params = self.chat_params(max_tokens, safe, temperature, top_p, top_k, seed, logprobs, guide, **fields)
        ids = self.chat_ids(messages)
        seq = self.engine.submit(ids, params, done, forced_prefix=self._forced if safe else None,
                                 on_tokens=on_tokens)
        return seq, len(ids)

    async def _submit_chat(self, messages, done, on_tokens, *args, **fields):
        if not self._started:
            await self.start()
        src = [fields.pop(k, None) for k in ("guided_regex", "guided_choice", "guided_json", "json_object")]
        guide = None
        if any(x is not None and x is not False for x in src):
            # on a worker thread; the submission stays here, so a request cancelled meanwhile is never submitted
            guide = await asyncio.get_running_loop().run_in_executor(None, self.compile_guide, *src)
        return self.submit_chat(messages, done, on_tokens, *args, guide=guide, **fields)

    async def _chat(self, messages, max_tokens, safe, temperature, top_p, top_k, seed, logprobs, **fields):
        """Submit one chat request and wait for it -> (finished sequence, prompt tokens)."""
        loop = asyncio.get_running_loop()
        fut: asyncio.Future = loop.create_future()
        seq, n_in = await self._submit_chat(messages, lambda sq: loop.call_soon_threadsafe(_resolve, fut, sq), None,
                                            max_tokens, safe, temperature, top_p, top_k, seed, logprobs, **fields)
        try:
            seq = await fut
        except asyncio.CancelledError:
            self.engine.abort(seq)
            raise
        if seq.error is not None:
            raise LLMUnavailableError(str(seq.error))
        return seq, n_in


def _logprob_entry(tok, tid: int, rec) -> dict:
    """OpenAI's `logprobs.content` entry of one generated token; rec = (logprob, top ids, top logprobs)."""
    def entry(i: int, lp: float) -> dict:
        return {"token": tok.decode([i]), "logprob": lp, "bytes": list(tok.token_bytes(i))}

    e = entry(tid, rec[0])
    e["top_logprobs"] = [entry(i, l) for i, l in zip(rec[1], rec[2]) if i >= 0]
    return e


def assemble_chat(tok, output_ids, n_forced, logprobs, finish_reason, stop_cut, n_in):
    """A finished chat sequence's data -> (text, finish_reason, prompt tokens, completion tokens, logprob entries
    or None): the one definition of a chat result, for the in-process backend and for the replica router
    (parallel/dp.py).  The text is the output's bytes without EOS, up to `stop_cut` when a stop string matched;
    `logprobs` (one record per token of output_ids[n_forced:], or None) gives an entry per token that is not EOS
    and starts before the cut.  The completion tokens count every output token: the one that completed a stop
    string counts, as EOS does."""
    pieces = [tok.token_bytes(t) if not tok.is_eos(t) else b"" for t in output_ids]
    data = b"".join(pieces)
    text = (data if stop_cut is None else data[:stop_cut]).decode("utf-8", "replace")
    content = None
    if logprobs is not None:
        content = []
        at = sum(len(p) for p in pieces[:n_forced])
        for tid, piece, rec in zip(output_ids[n_forced:], pieces[n_forced:], logprobs):
            if not tok.is_eos(tid) and (stop_cut is None or at < stop_cut):
                content.append(_logprob_entry(tok, tid, rec))
            at += len(piece)
    return text, ("stop" if finish_reason == "stop" else "length"), n_in, len(output_ids), content


class ChatStream:
    """The events of a streamed chat completion from its tokens as they settle (EngineLLM.stream_chat and the
    router's): `push` the ids of one engine step with their logprob records (or None) -> {"text", "logprobs"} or
    None when nothing can be released yet; `finish` -> the last content event, if any, and the closing one."""

    def __init__(self, tok, stops, logprobs: bool = False, forced_ids=()):
        self.tok = tok
        self.logprobs = logprobs
        self.dec = StreamDecoder(stops)
        self.entries: list = []   # per fed token: its tid and record, None for a token that has no entry
        self.sent = 0             # entries that left (StreamDecoder.tokens: with their token's first byte)
        self.text = ""            # of the jump-forward prefix, released with the first event
        for t in forced_ids:
            self._feed(t, None)

    def _feed(self, tid, rec) -> None:
        if self.tok.is_eos(tid):
            return
        self.entries.append(None if rec is None else (tid, rec))
        text, _ = self.dec.feed(self.tok.token_bytes(tid))
        self.text += text

    def _event(self):
        took, self.sent = self.entries[self.sent:self.dec.tokens], self.dec.tokens
        text, self.text = self.text, ""
        content = [_logprob_entry(self.tok, *e) for e in took if e is not None]
        if not text and not content:
            return None
        return {"text": text, "logprobs": content if self.logprobs else None}

    def push(self, ids, recs, emit: bool = True):
        """emit=False: the sequence has finished, `finish` follows and carries what these tokens release (so a
        step yields at most one content event)."""
        for i, t in enumerate(ids):
            self._feed(t, recs[i] if recs is not None else None)
        return self._event() if emit else None

    def finish(self, finish_reason, n_out):
        text, _ = self.dec.finish()
        self.text += text
        ev = self._event()
        last = {"finish_reason": "stop" if finish_reason == "stop" else "length", "stop_reason": self.dec.match,
                "completion_tokens": n_out}
        return [last] if ev is None else [ev, last]


def _resolve(fut: asyncio.Future, seq) -> None:
    if not fut.done():
        fut.set_result(seq)
