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
        return cls(eng, max_new_tokens=settings.MAX_NEW_TOKENS, ignore_eos=settings.IGNORE_EOS,
                   safe_decode=settings.SAFE_DECODE)

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
                            top_p: float = 1.0, top_k: int = 0, seed: Optional[int] = None, **penalties):
        """Returns (text, finish_reason, prompt_tokens, completion_tokens).  temperature 0 (the default)
        decodes greedily; above it the engine samples (top_k / top_p cuts, `seed` makes it repeatable).
        penalties: presence_penalty, frequency_penalty, repetition_penalty, logit_bias ({token id: bias}),
        applied to the logits before the token is chosen, also at temperature 0 (SamplingParams); and
        guided_regex or guided_choice: the completion then matches the pattern / is one of the choices when it
        ends with "stop", and is a prefix of a match when max_tokens cuts it (engine/guided.py); json_object=True
        (any JSON object) or guided_json (a JSON Schema of the supported subset, dict or string): JSON mode.
        Raises ValueError for a request the engine cannot serve (temperature > 0, penalties or a guide under
        TP > 1, a logit_bias id outside the vocabulary, a pattern outside the dialect or that the tokenizer
        cannot spell, a full guide table)."""
        seq, n_in = await self._chat(messages, max_tokens, safe, temperature, top_p, top_k, seed, None, **penalties)
        out = [t for t in seq.output_ids if not self.tok.is_eos(t)]
        return self.tok.decode(out), ("stop" if seq.finish_reason == "stop" else "length"), n_in, len(seq.output_ids)

    async def generate_chat_logprobs(self, messages, top_logprobs: int = 0, max_tokens: int = 64, safe: bool = False,
                                     temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0,
                                     seed: Optional[int] = None, **penalties):
        """generate_chat with per-token log-probabilities: returns its four values and OpenAI's
        `logprobs.content` list, one {"token", "logprob", "bytes", "top_logprobs": [{"token", "logprob",
        "bytes"}, ...]} per model-generated token that makes up the text (the stripped EOS and a
        jump-forward prefix have none), with `top_logprobs` (0..20) alternatives each.  The values are
        the model's distribution under the token mask before temperature / top_k / top_p and before the
        penalties and logit_bias (ops.token_logprobs): a token's logprob is its raw one.
        Raises ValueError under TP > 1."""
        seq, n_in = await self._chat(messages, max_tokens, safe, temperature, top_p, top_k, seed, int(top_logprobs),
                                     **penalties)
        tok = self.tok
        out = [t for t in seq.output_ids if not tok.is_eos(t)]

        def entry(tid: int, lp: float) -> dict:
            return {"token": tok.decode([tid]), "logprob": lp, "bytes": list(tok.token_bytes(tid))}

        content = []
        for tid, rec in zip(seq.generated, seq.logprobs):
            if tok.is_eos(tid):
                continue
            e = entry(tid, rec.logprob)
            e["top_logprobs"] = [entry(i, l) for i, l in zip(rec.top_ids, rec.top_logprobs) if i >= 0]
            content.append(e)
        return (tok.decode(out), ("stop" if seq.finish_reason == "stop" else "length"), n_in, len(seq.output_ids),
                content)

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

    async def _chat(self, messages, max_tokens, safe, temperature, top_p, top_k, seed, logprobs,
                    presence_penalty: float = 0.0, frequency_penalty: float = 0.0, repetition_penalty: float = 1.0,
                    logit_bias=None, guided_regex: Optional[str] = None, guided_choice: Optional[List[str]] = None,
                    guided_json=None, json_object: bool = False):
        """Submit one chat request and wait for it -> (finished sequence, prompt tokens)."""
        if not self._started:
            await self.start()
        loop = asyncio.get_running_loop()
        guide = None
        if guided_regex is not None or guided_choice is not None or guided_json is not None or json_object:
            guide = await loop.run_in_executor(None, self.compile_guide, guided_regex, guided_choice, guided_json,
                                               json_object)
        fut: asyncio.Future = loop.create_future()
        params = SamplingParams(max_new_tokens=max_tokens, ignore_eos=False, safe_decode=safe,
                                temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=seed,
                                logprobs=logprobs, presence_penalty=float(presence_penalty),
                                frequency_penalty=float(frequency_penalty),
                                repetition_penalty=float(repetition_penalty),
                                logit_bias={int(t): float(b) for t, b in logit_bias.items()} if logit_bias else None,
                                guide=guide)
        ids = self.chat_ids(messages)
        seq = self.engine.submit(ids, params, lambda sq: loop.call_soon_threadsafe(_resolve, fut, sq),
                                 forced_prefix=self._forced if safe else None)
        try:
            seq = await fut
        except asyncio.CancelledError:
            self.engine.abort(seq)
            raise
        if seq.error is not None:
            raise LLMUnavailableError(str(seq.error))
        return seq, len(ids)


def _resolve(fut: asyncio.Future, seq) -> None:
    if not fut.done():
        fut.set_result(seq)
