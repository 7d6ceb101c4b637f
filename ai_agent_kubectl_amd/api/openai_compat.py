"""OpenAI-compatible `/v1/chat/completions` and `/v1/models` served by the on-node engine.

The reference is an OpenAI *client* (`ChatOpenAI`, `/root/reference/app.py:117`).  Exposing the same
wire format from this service lets existing OpenAI-speaking clients (including another copy of the
reference pointed at `OPENAI_BASE_URL=http://<this host>/v1`, or this framework's own
`LLM_BACKEND=openai`) use the MI355X engine directly.  `temperature` (0..2, default 0 = greedy, what
the reference always used, app.py:109), `top_p` (0 < p <= 1), `top_k` (>= 0, 0 = off) and `seed` are
honoured: above temperature 0 the engine samples by seeded Gumbel-max (csrc/sampling_stochastic.hip),
and the same seed, prompt and parameters give the same completion whatever else is in the batch;
without a seed every request draws its own.  Out-of-range values get 422; temperature > 0 on a
tensor-parallel engine gets 400.  `max_tokens` caps the completion.
`logprobs: true` adds `choices[0].logprobs.content` in OpenAI's shape, one entry per token of the
content, each with `top_logprobs` (0..20) alternatives (csrc/logprobs.hip).  They are the model's
distribution under the token mask BEFORE temperature / top_p / top_k are applied (what vLLM reports by
default), so they do not depend on those fields or on `seed`.  `top_logprobs` without `logprobs: true`
gets 422; logprobs on a tensor-parallel engine get 400.
`presence_penalty`, `frequency_penalty` (-2..2), `repetition_penalty` (0 < r <= 2, the vLLM / HF extension) and
`logit_bias` ({"<token id>": -100..100}, at most 300 entries) edit the logits before the token is chosen, also
at temperature 0 (csrc/logit_adjust.hip); `logprobs` stay the model's raw ones.  Out-of-range values and
non-integer keys get 422; a token id past the vocabulary and any of the four on a tensor-parallel engine get 400.
`guided_regex` (a pattern of at most 2048 characters) or `guided_choice` (1..256 strings of 1..256 bytes), vLLM's
fields, constrain the completion (engine/guided.py, csrc/guide_mask.hip): with finish_reason "stop" the content
matches the pattern / is one of the choices, with "length" it is a prefix of a match.  Both together, an empty
string or list and a cap violation get 422; a pattern outside the dialect, one the tokenizer cannot spell, a full
guide table and a tensor-parallel engine get 400.
JSON mode (engine/guided.py, csrc/guide_stack.hip): `response_format: {"type": "json_object"}` constrains the content
to one RFC 8259 object, `{"type": "json_schema", "json_schema": {"name": .., "schema": {..}}}` and vLLM's
`guided_json` (a dict or a JSON string, at most 16 KiB) to the supported subset of JSON Schema; `{"type": "text"}` is
the default.  An unknown type, a missing or non-object schema, an oversized schema and any two of response_format,
guided_json, guided_regex and guided_choice get 422; a schema outside the subset gets 400 like a bad pattern.
`stop` (a string or a list of 1..4 strings, each 1..64 bytes of UTF-8; anything else gets 422) ends the completion
before the first of them that occurs in it, with finish_reason "stop" (engine/streaming.py); it combines with every
other field.  A request that sent `stop` also gets vLLM's `choices[0].stop_reason`: the matched string, or null for
EOS or length.
`stream: true` answers with server-sent events (`text/event-stream`): chunks of `object: "chat.completion.chunk"`
that share `id`, `created` and `model`; the first one's delta is {"role": "assistant", "content": ""}, then content
chunks (with `logprobs: {"content": [...]}` when asked: an entry leaves with the first byte of its token), then one
with `delta: {}` and the `finish_reason` (and `stop_reason` under the rule above), then `data: [DONE]`.  With
`stream_options: {"include_usage": true}` a last chunk with `choices: []` and `usage` comes before [DONE] and every
other chunk carries `"usage": null`; `stream_options` without `stream` gets 422.  The deltas join to exactly the
content, and the entries to exactly the logprobs, of the same request without `stream`.  What fails before the
first byte (422, 400, 503) is a plain HTTP error; a failure afterwards is one `data: {"error": {...}}` event and the
stream ends without [DONE].  A client that disconnects aborts its request.
Auth: when API_AUTH_KEY is set, `Authorization: Bearer <key>` or `X-API-Key: <key>`.
"""
from __future__ import annotations

import time
import uuid
import json
from typing import Any, Dict, List, Optional, Union

from fastapi import Header, HTTPException, Request
from fastapi.responses import StreamingResponse
from pydantic import BaseModel, Field, field_validator, model_validator

from ..llm.base import LLMUnavailableError


class ChatMessage(BaseModel):
    role: str
    content: str


class ChatRequest(BaseModel):
    model: Optional[str] = None
    messages: List[ChatMessage] = Field(..., min_length=1)
    max_tokens: Optional[int] = Field(None, ge=1, le=4096)
    temperature: Optional[float] = Field(0.0, ge=0, le=2)
    top_p: Optional[float] = Field(1.0, gt=0, le=1)
    top_k: Optional[int] = Field(0, ge=0)
    seed: Optional[int] = None
    stream: Optional[bool] = False
    logprobs: Optional[bool] = False
    top_logprobs: Optional[int] = Field(None, ge=0, le=20)
    presence_penalty: Optional[float] = Field(0.0, ge=-2.0, le=2.0)
    frequency_penalty: Optional[float] = Field(0.0, ge=-2.0, le=2.0)
    repetition_penalty: Optional[float] = Field(1.0, gt=0.0, le=2.0)
    logit_bias: Optional[Dict[str, float]] = None   # OpenAI's wire form: decimal token-id strings -> bias
    guided_regex: Optional[str] = Field(None, min_length=1, max_length=2048)
    guided_choice: Optional[List[str]] = Field(None, min_length=1, max_length=256)
    guided_json: Optional[Union[Dict[str, Any], str]] = None
    response_format: Optional[Dict[str, Any]] = None
    stop: Optional[Union[str, List[str]]] = None
    stream_options: Optional[Dict[str, Any]] = None

    @field_validator("stop")
    @classmethod
    def _stop_entries(cls, v):
        if v is None:
            return v
        stops = [v] if isinstance(v, str) else v
        if not 1 <= len(stops) <= 4:
            raise ValueError("stop accepts a string or 1..4 strings")
        for s in stops:
            try:
                n = len(s.encode("utf-8"))
            except UnicodeEncodeError:
                raise ValueError("every stop string must be UTF-8") from None
            if not 1 <= n <= 64:
                raise ValueError("every stop string must be 1..64 bytes long")
        return stops

    @field_validator("guided_json")
    @classmethod
    def _guided_json_schema(cls, v):
        if v is None:
            return v
        if isinstance(v, str):
            try:
                parsed = json.loads(v)
            except ValueError:
                raise ValueError("guided_json must be a JSON Schema object or its JSON text")
            if not isinstance(parsed, dict):
                raise ValueError("guided_json must be a JSON Schema object")
        if len((v if isinstance(v, str) else json.dumps(v, ensure_ascii=False)).encode("utf-8")) > MAX_SCHEMA_BYTES:
            raise ValueError(f"guided_json accepts at most {MAX_SCHEMA_BYTES} bytes of schema")
        return v

    @field_validator("response_format")
    @classmethod
    def _response_format_shape(cls, v):
        if v is None:
            return v
        kind = v.get("type")
        if kind not in ("text", "json_object", "json_schema"):
            raise ValueError("response_format.type must be text, json_object or json_schema")
        if kind == "json_schema":
            js = v.get("json_schema")
            if not isinstance(js, dict) or not isinstance(js.get("schema"), dict):
                raise ValueError("response_format.json_schema.schema must be a JSON Schema object")
            if len(json.dumps(js["schema"], ensure_ascii=False).encode("utf-8")) > MAX_SCHEMA_BYTES:
                raise ValueError(f"response_format.json_schema.schema accepts at most {MAX_SCHEMA_BYTES} bytes")
        return v

    @field_validator("guided_choice")
    @classmethod
    def _guided_choice_entries(cls, v):
        for c in v or ():
            if not 1 <= len(c.encode("utf-8")) <= 256:
                raise ValueError("every guided_choice entry must be 1..256 bytes long")
        return v

    @field_validator("logit_bias")
    @classmethod
    def _logit_bias_entries(cls, v):
        if v is None:
            return v
        if len(v) > 300:
            raise ValueError("logit_bias accepts at most 300 entries")
        for key, b in v.items():
            if not (key.isascii() and key.isdigit()):
                raise ValueError(f"logit_bias key {key!r} is not a token id")
            if not -100.0 <= b <= 100.0:
                raise ValueError(f"logit_bias value for token {key} must be in -100..100")
        return v

    @model_validator(mode="after")
    def _top_logprobs_needs_logprobs(self):
        if self.top_logprobs is not None and not self.logprobs:
            raise ValueError("top_logprobs requires logprobs: true")
        if self.stream_options is not None and not self.stream:
            raise ValueError("stream_options requires stream: true")
        if self.guided_regex is not None and self.guided_choice is not None:
            raise ValueError("guided_regex and guided_choice cannot be combined")
        structured = self.response_format is not None and self.response_format.get("type") != "text"
        if structured + (self.guided_json is not None) + (self.guided_regex is not None) + (self.guided_choice is not None) > 1:
            raise ValueError("response_format, guided_json, guided_regex and guided_choice cannot be combined")
        return self


MAX_SCHEMA_BYTES = 16384   # engine/guided.py MAX_SCHEMA_BYTES

_NEUTRAL = dict(presence_penalty=0.0, frequency_penalty=0.0, repetition_penalty=1.0, logit_bias=None)


def install(app, svc, settings) -> None:
    from ..models.lora import parse_adapters
    backend = svc.backend
    if backend is None or not hasattr(backend, "generate_chat"):
        return

    # the LoRA adapters in slot order (models/lora.py): a request whose `model` names one runs on it
    adapters = [name for name, _ in parse_adapters(getattr(settings, "LORA_ADAPTERS", ""))]

    def _auth(authorization: Optional[str], x_api_key: Optional[str]) -> None:
        key = settings.API_AUTH_KEY
        if not key:
            return
        bearer = authorization[7:] if authorization and authorization.lower().startswith("bearer ") else None
        if bearer != key and x_api_key != key:
            raise HTTPException(status_code=401, detail="Invalid API Key")

    @app.get("/v1/models")
    async def list_models(authorization: Optional[str] = Header(None), x_api_key: Optional[str] = Header(None)):
        _auth(authorization, x_api_key)
        data = [{"id": settings.MODEL, "object": "model", "owned_by": "local"}]
        data += [{"id": name, "object": "model", "owned_by": "local", "parent": settings.MODEL} for name in adapters]
        return {"object": "list", "data": data}

    async def _stream(req: ChatRequest, request: Request, msgs, kw, head):
        """`stream: true`.  The backend's first event is awaited before the response starts, so a request that the
        engine refuses is a plain 400 / 503."""
        if not hasattr(backend, "stream_chat"):
            raise HTTPException(status_code=400, detail="this backend does not stream")
        kw.pop("with_stop", None)
        events = backend.stream_chat(msgs, top_logprobs=(req.top_logprobs or 0) if req.logprobs else None, **kw)
        try:
            first = await events.__anext__()
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        except LLMUnavailableError as e:
            raise HTTPException(status_code=503, detail=str(e))
        usage = bool((req.stream_options or {}).get("include_usage"))

        def chunk(choices, **extra) -> bytes:
            body = dict(head, object="chat.completion.chunk", choices=choices, **extra)
            if usage and "usage" not in body:
                body["usage"] = None
            return b"data: " + json.dumps(body, ensure_ascii=False).encode("utf-8", "replace") + b"\n\n"

        async def body():
            try:
                yield chunk([{"index": 0, "delta": {"role": "assistant", "content": ""}, "finish_reason": None}])
                n_out = 0
                async for ev in events:
                    if "finish_reason" in ev:
                        last = {"index": 0, "delta": {}, "finish_reason": ev["finish_reason"]}
                        if req.stop is not None:
                            at = ev["stop_reason"]
                            last["stop_reason"] = req.stop[at] if at is not None else None
                        n_out = ev["completion_tokens"]
                        yield chunk([last])
                        continue
                    ch = {"index": 0, "delta": {"content": ev["text"]}, "finish_reason": None}
                    if ev["logprobs"] is not None:
                        ch["logprobs"] = {"content": ev["logprobs"]}
                    yield chunk([ch])
                if usage:
                    n_in = first["prompt_tokens"]
                    yield chunk([], usage={"prompt_tokens": n_in, "completion_tokens": n_out,
                                           "total_tokens": n_in + n_out})
                yield b"data: [DONE]\n\n"
            except Exception as e:   # after the first byte: one error event, and no [DONE]
                kind = "service_unavailable" if isinstance(e, LLMUnavailableError) else "internal_error"
                yield b"data: " + json.dumps({"error": {"message": str(e), "type": kind}}).encode() + b"\n\n"
            finally:
                await events.aclose()   # a client that went away: the backend aborts the request

        return StreamingResponse(body(), media_type="text/event-stream", headers={"Cache-Control": "no-cache"})

    @app.post("/v1/chat/completions")
    async def chat_completions(req: ChatRequest, request: Request, authorization: Optional[str] = Header(None),
                               x_api_key: Optional[str] = Header(None)):
        _auth(authorization, x_api_key)
        msgs = [m.model_dump() for m in req.messages]
        kw = dict(max_tokens=req.max_tokens or 64, temperature=req.temperature or 0.0,
                  top_p=1.0 if req.top_p is None else req.top_p, top_k=req.top_k or 0, seed=req.seed)
        bias = {int(t): b for t, b in (req.logit_bias or {}).items()}
        pen = dict(presence_penalty=req.presence_penalty or 0.0, frequency_penalty=req.frequency_penalty or 0.0,
                   repetition_penalty=1.0 if req.repetition_penalty is None else req.repetition_penalty,
                   logit_bias=bias or None)
        if pen != _NEUTRAL:   # only when sent: a plain request is submitted exactly as it always was
            kw.update(pen)
        if req.guided_regex is not None:
            kw["guided_regex"] = req.guided_regex
        if req.guided_choice is not None:
            kw["guided_choice"] = list(req.guided_choice)
        if req.guided_json is not None:
            kw["guided_json"] = req.guided_json
        fmt = (req.response_format or {}).get("type", "text")
        if fmt == "json_object":
            kw["json_object"] = True
        elif fmt == "json_schema":
            kw["guided_json"] = req.response_format["json_schema"]["schema"]
        if req.model in adapters:   # any other name: the base model, the name echoed
            kw["adapter"] = adapters.index(req.model)
        if req.stop is not None:   # only when sent, like the penalties
            kw.update(stop=[s.encode("utf-8") for s in req.stop], with_stop=True)
        head = {"id": "chatcmpl-" + uuid.uuid4().hex[:24], "created": int(time.time()),
                "model": req.model or settings.MODEL}
        if req.stream:
            return await _stream(req, request, msgs, kw, head)
        content, matched = None, None
        try:
            if req.logprobs:
                if not hasattr(backend, "generate_chat_logprobs"):
                    raise ValueError("this backend does not report logprobs")
                text, finish, n_in, n_out, content, *matched = await backend.generate_chat_logprobs(
                    msgs, top_logprobs=req.top_logprobs or 0, **kw)
            else:
                text, finish, n_in, n_out, *matched = await backend.generate_chat(msgs, **kw)
        except ValueError as e:   # a request this engine cannot serve (sampling / logprobs / penalties / guides under TP > 1, a bad pattern)
            raise HTTPException(status_code=400, detail=str(e))
        except LLMUnavailableError as e:
            raise HTTPException(status_code=503, detail=str(e))
        choice = {"index": 0, "message": {"role": "assistant", "content": text}, "finish_reason": finish}
        if content is not None:   # only when asked for: the response is otherwise what it always was
            choice["logprobs"] = {"content": content}
        if req.stop is not None:
            choice["stop_reason"] = req.stop[matched[0]] if matched[0] is not None else None
        return {
            "id": head["id"], "object": "chat.completion", "created": head["created"],
            "model": head["model"],
            "choices": [choice],
            "usage": {"prompt_tokens": n_in, "completion_tokens": n_out, "total_tokens": n_in + n_out},
        }
