"""Request / sequence state shared by the scheduler, the runner and the engine loop."""
from __future__ import annotations

import enum
import itertools
import random
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, NamedTuple, Optional

_ids = itertools.count()

# token id of an output whose value is still on the device: a step scheduled while the previous
# one is in flight (engine._lookahead_step) appends it; the readback replaces it, and until then the
# next step's packed inputs take that token from the device (runner fixups)
PLACEHOLDER = -1
ADAPTER_TAG_SHIFT = 20   # Sequence.cache_ids


class SeqStatus(enum.Enum):
    WAITING = 0
    RUNNING = 1
    FINISHED = 2
    ABORTED = 3


@dataclass
class SamplingParams:
    max_new_tokens: int = 24
    ignore_eos: bool = False
    safe_decode: bool = True      # SAFE_DECODE token mask (engine/safe_decode.py)
    # seeded sampling (csrc/sampling_stochastic.hip); the defaults are greedy decoding
    temperature: float = 0.0      # 0 = greedy (top_k / top_p / seed then have no effect)
    top_k: int = 0                # 0 = off
    top_p: float = 1.0            # 1 = off
    seed: Optional[int] = None    # None: a random 64-bit seed per sequence (Sequence.sample_seed)
    # per-token log-probabilities (csrc/logprobs.hip): None = off, 0..20 = the number of alternatives
    # reported beside every generated token.  They describe the model's distribution under the
    # SAFE_DECODE mask before temperature / top_k / top_p, so those fields do not change them
    logprobs: Optional[int] = None
    # edits of the logits before the sampler reads them (csrc/logit_adjust.hip; ops/reference.py
    # `logit_adjust` defines them), also at temperature 0.  c = a token's occurrences in the output so far
    presence_penalty: float = 0.0     # -2..2: subtracted once from every token with c > 0
    frequency_penalty: float = 0.0    # -2..2: times c, subtracted
    repetition_penalty: float = 1.0   # 0 < r <= 2 (vLLM / HF): a token of the prompt or the output: l / r if l > 0 else l * r
    logit_bias: Optional[Dict[int, float]] = None   # token id -> -100..100, at most 300 entries; added last
    # guided decoding (csrc/guide_mask.hip): a compiled engine/guided.py Guide (compile_regex / compile_choice);
    # every step's token mask then also admits only tokens that keep the output a prefix of a match
    guide: Optional[object] = None
    # 1..4 byte strings of 1..64 bytes (engine/streaming.py): the sequence finishes with "stop" at the first token
    # after which one of them occurs in the output's bytes, and its content ends where that match starts
    # (Sequence.stop_cut).  Sampling does not see it: up to the cut the output is the output without `stop`
    stop: Optional[List[bytes]] = None
    # the LoRA adapter the request runs on: its slot among the engine's loaded adapters (models/lora.py), None = the
    # base model.  Static for the sequence's life
    adapter: Optional[int] = None

    @property
    def penalised(self) -> bool:
        """Any of the four fields is not neutral: the request's steps take the penalty route."""
        return (self.presence_penalty != 0 or self.frequency_penalty != 0 or self.repetition_penalty != 1
                or bool(self.logit_bias))


class TokenLogprob(NamedTuple):
    """The record of one model-generated token (Sequence.logprobs)."""
    logprob: float            # of the chosen token
    top_ids: List[int]        # the request's `logprobs` most likely tokens, -1 past the allowed count
    top_logprobs: List[float]


@dataclass(eq=False)   # identity semantics: `seq in list` / `remove` must not compare token lists
class Sequence:
    prompt_ids: List[int]
    params: SamplingParams
    callback: Optional[Callable[["Sequence"], None]] = None
    forced_prefix: List[int] = field(default_factory=list)   # jump-forward tokens (counted as output)
    seq_id: int = field(default_factory=lambda: next(_ids))
    status: SeqStatus = SeqStatus.WAITING
    output_ids: List[int] = field(default_factory=list)
    block_table: List[int] = field(default_factory=list)
    block_hashes: List[int] = field(default_factory=list)
    num_computed: int = 0           # tokens whose KV is in the cache
    num_cached_prompt: int = 0      # prompt tokens served by the prefix cache
    n_forced: int = 0
    finish_reason: Optional[str] = None
    error: Optional[BaseException] = None
    t_arrival: float = field(default_factory=time.perf_counter)
    t_scheduled: Optional[float] = None     # first admission into a prefill step (queue wait ends)
    t_first_token: Optional[float] = None
    t_finish: Optional[float] = None
    ph_row: Optional[int] = None            # row of the in-flight step whose token is the PLACEHOLDER
    sample_seed: int = 0                    # the 64 bits the sampling noise is keyed with (params.seed or random)
    # params.logprobs is set: one TokenLogprob per model-generated token, aligned with `generated`
    # (the jump-forward prefix has none); appended where the token's placeholder is settled
    logprobs: List[TokenLogprob] = field(default_factory=list)
    # params.penalised: the per-sequence part of the penalty image (engine/penalties.py PenaltyState)
    penalty_state: Optional[object] = None
    # params.guide: the DFA state after the final output tokens (engine/guided.py GuideState) and the
    # guide's placement in the device arena (GuideTable.acquire; released when the sequence leaves)
    guide_state: Optional[object] = None
    guide_ref: Optional[object] = None
    # params.stop: the scanner over the output's bytes (engine/streaming.py StopScanner), and once a stop string
    # matched the byte offset where the content ends and the index of the string that matched there
    stop_scan: Optional[object] = None
    stop_cut: Optional[int] = None
    stop_match: Optional[int] = None
    # streaming: called on the engine thread after every step that settled a token of this sequence, with the
    # sequence and the index in `output_ids` of its first newly settled token.  It must not block
    on_tokens: Optional[Callable[["Sequence", int], None]] = None

    def __post_init__(self):
        seed = self.params.seed if self.params.seed is not None else random.getrandbits(64)
        self.sample_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.n_forced = len(self.forced_prefix)
        if self.forced_prefix:
            # jump-forward: deterministic constrained tokens are appended to the prompt and also
            # reported as the first output tokens (equivalent to decoding them under the mask).
            self.prompt_ids = list(self.prompt_ids) + list(self.forced_prefix)
            self.output_ids = list(self.forced_prefix)

    @property
    def generated(self) -> List[int]:
        return self.output_ids[self.n_forced:]

    @property
    def all_ids(self) -> List[int]:
        return self.prompt_ids + self.output_ids[self.n_forced:]

    @property
    def cache_ids(self) -> List[int]:
        """all_ids as the prefix cache sees them: KV computed under an adapter must never be shared with the base
        model or another adapter, so adapter a's ids carry the tag (a + 1) << 20 (the vocabulary is below 2**20:
        models/lora.py load_adapters refuses a larger one)."""
        a = self.params.adapter
        if a is None:
            return self.all_ids
        tag = (int(a) + 1) << ADAPTER_TAG_SHIFT
        return [t + tag for t in self.all_ids]

    @property
    def total_len(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids) - self.n_forced

    @property
    def num_generated(self) -> int:
        """Tokens produced by the model (excluding the jump-forward prefix)."""
        return len(self.output_ids) - self.n_forced

    @property
    def finished(self) -> bool:
        return self.status in (SeqStatus.FINISHED, SeqStatus.ABORTED)
