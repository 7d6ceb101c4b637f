"""Model runner: KV cache ownership, step metadata, eager prefill, hipGraph decode, TP fan-out.

Decode steps dominate the request latency (one replay per output token, SURVEY.md §3.6 hot loop 1),
so they are captured once per batch bucket (`HIPGRAPH_BUCKETS`) with `torch.cuda.CUDAGraph` (a
hipGraph on ROCm): embedding -> 32 x (norm, QKV GEMM, RoPE+KV append, paged decode attention, O
GEMM [+ all-reduce], norm, gate_up GEMM, SiLU*mul, down GEMM [+ all-reduce]) -> norm -> LM head ->
masked argmax [+ all-gather].  All per-step inputs live in ONE device staging tensor at fixed
offsets so a step is: one pinned host->device copy, one graph replay, one 4*B-byte readback.

With TP > 1 the driver rank (rank 0) owns the scheduler; every step it broadcasts a small header
and the packed metadata and all ranks run the same forward, the collectives
inside it synchronising them.  Worker ranks sit in `worker_loop()`.
"""
from __future__ import annotations

import bisect
import logging
import os
import threading
import time
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from ..models.config import ModelConfig
from .. import ops
from ..models.llama import SAMP_WORDS, AttnMeta, GuideArrays, LlamaModel, LogitEdits, SampleArrays
from ..ops.autotune import tune_engine

logger = logging.getLogger("app.engine")
from ..parallel.comm import LocalComm
from .guided import GUIDE_STATES, GuideTable, StackGuide, pack_guide_stacks, pack_guides
from .penalties import pack_edits
from .safe_decode import mask_index_for
from .scheduler import Batch
from .sequence import PLACEHOLDER

KIND_STOP, KIND_DECODE, KIND_PREFILL = 0, 1, 2
HDR = 8
LP_WORDS = 1 + 2 * ops.MAX_TOP_LOGPROBS   # int32 words per row of a log-probability image at the largest top_n


class CollectiveTimeout(RuntimeError):
    """A one-shot TP collective gave up waiting for a peer (csrc/allreduce.hip's bounded spin set its
    error word): the step's reduced values are stale, so its tokens must not be used.  Fatal for
    the process (the TP group's collective epochs are out of step): engine.py fails the in-flight
    requests with 503 and marks the engine unhealthy / exits for the supervisor to restart it."""


def shared_prefix_len(bt: np.ndarray, lim: int) -> int:
    """Length of the common prefix of the rows of `bt` ([B, max_blocks]) within the first `lim` columns."""
    if lim <= 0 or bt.shape[0] == 0:
        return 0
    eq = (bt[:, :lim] == bt[0:1, :lim]).all(axis=0)
    return lim if bool(eq.all()) else int(np.argmin(eq))


class PersistentStall(RuntimeError):
    """The batch-1 persistent decode kernel (csrc/decode_persistent.hip) gave up a grid-wide wait:
    some workgroup never ran (the GPU shared with another kernel), so the step's hidden state is
    stale.  Recoverable: the engine fails the in-flight requests and recovers; the runner has
    already switched batch-1 decode back to the per-kernel chain."""


class StepHandle(NamedTuple):
    """A step queued on the device and not yet read back (`collect`)."""
    event: Optional["torch.cuda.Event"]   # recorded after the step's token readback copy
    host_out: torch.Tensor                # pinned host buffer the sampled tokens land in
    rows: int
    t0: float                             # perf_counter at launch
    prefill_tokens: int = 0               # > 0: a prefill step (launch_prefill_async)
    progress: Optional["torch.cuda.Event"] = None   # recorded KA_LOOKAHEAD_LAYERS layers before the end
    err_host: Optional[torch.Tensor] = None   # pinned copy of the one-shot collectives' error word
    lp_host: Optional[torch.Tensor] = None    # pinned [rows, 1 + 2 * lp_n] image of the step's log-probabilities
    lp_n: int = 0                             # alternatives per row in lp_host


class StepLogprobs(NamedTuple):
    """A step's log-probability records on the host, by batch row (engine._settle takes the rows of
    the requests that asked)."""
    logprob: np.ndarray        # fp32 [rows]
    top_ids: np.ndarray        # int32 [rows, n]
    top_logprobs: np.ndarray   # fp32 [rows, n]


class ModelRunner:
    def __init__(self, cfg: ModelConfig, weights: Dict[str, torch.Tensor], device: torch.device,
                 num_blocks: int, block_size: int = 16, max_model_len: int = 4096, graph_buckets=(1, 2, 4, 8),
                 mask_bits: Optional[np.ndarray] = None, comm=None, tp_rank: int = 0, tp_size: int = 1,
                 ep_rank: int = 0, ep_size: int = 1, use_graphs: bool = True, tokenizer=None,
                 guide_states: int = GUIDE_STATES):
        self.cfg = cfg
        self.device = torch.device(device)
        self.comm = comm or LocalComm()
        # mixed steps: decode rows through the decode kernel (KA_SPLIT_MIXED_ATTN=0: all varlen)
        self.split_mixed_attention = os.environ.get("KA_SPLIT_MIXED_ATTN", "1") == "1"
        self.prefill_pad = int(os.environ.get("KA_PREFILL_PAD", "256"))
        self.prefill_pad_min = int(os.environ.get("KA_PREFILL_PAD_MIN", "1024"))
        # an async prefill / mixed step records a progress event this many layers before its end: the
        # engine schedules the step after it once that event has passed (engine._lookahead_step)
        self.lookahead_layers = int(os.environ.get("KA_LOOKAHEAD_LAYERS", "10"))
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.model = LlamaModel(cfg, weights, self.comm, tp_rank, tp_size, ep_rank, ep_size)
        self.block_size = block_size
        self.num_blocks = num_blocks
        self.max_blocks = (max_model_len + block_size - 1) // block_size
        hkv = cfg.num_kv_heads // tp_size
        L, D = cfg.num_layers, cfg.head_dim
        dt = weights["embed"].dtype
        # zero-filled: stale slots read by masked lanes must be finite (attention.hip contract)
        self.k_cache = torch.zeros((L, num_blocks, hkv, block_size, D), dtype=dt, device=self.device)
        self.v_cache = torch.zeros((L, num_blocks, hkv, D, block_size), dtype=dt, device=self.device)
        self.mask_bits = (torch.from_numpy(mask_bits.view(np.int32)).to(self.device)
                          if mask_bits is not None else None)
        self.buckets = sorted(set(int(b) for b in graph_buckets))
        self.bmax = self.buckets[-1] if self.buckets else 1
        self.use_graphs = use_graphs and self.device.type == "cuda"
        # ---- decode staging: [ids | pos | slots | ctx | mask | block_tables] at fixed offsets ----
        B = self.bmax
        # nsh: the leading block-table entries every row shares (cascade decode attention, 16-int slot)
        self._off = {"ids": 0, "pos": B, "slots": 2 * B, "ctx": 3 * B, "mask": 4 * B, "nsh": 5 * B, "bt": 5 * B + 16}
        self._stage_len = 5 * B + 16 + B * self.max_blocks
        # cascade decode attention from this bucket up (KA_CASCADE_MIN_B; 0 = off, the default): the
        # shared prefix blocks attended once per kv head and 16 query rows instead of once per row.
        # Measured slower at B = 64 / 256 with a 5-block shared prefix (+0.23 / +0.14 ms per step,
        # profiles/r4/cascade/): the per-row kernel's prefix reads are L2 hits, and the partials'
        # round trip plus the second launch cost more than they save.
        self.cascade_min_b = int(os.environ.get("KA_CASCADE_MIN_B", "0"))
        self.d_stage = torch.zeros(self._stage_len, dtype=torch.int32, device=self.device)
        pin = self.device.type == "cuda"
        self.h_stage = torch.zeros(self._stage_len, dtype=torch.int32, pin_memory=pin)
        self.h_np = self.h_stage.numpy()
        # overlapped decode (launch_decode_async): second pinned staging / output buffers so step
        # t+1 can be packed and queued while step t's copies are still in flight
        self._h_stages = [self.h_stage, torch.zeros(self._stage_len, dtype=torch.int32, pin_memory=pin)]
        self._h_outs = [torch.zeros(B, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._flip = 0
        self.d_logits_idx = torch.arange(B, dtype=torch.int64, device=self.device)
        self.d_out = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.h_out = torch.zeros(B, dtype=torch.int32, pin_memory=pin)
        # steps queued ahead of a readback (engine._lookahead_step): prefill / mixed staging in grown
        # pinned buffers and token outputs, each double-buffered (a buffer is reused two launches
        # later, when the step that used it has been read back), and the placeholder fixups of a
        # decode step ([dst rows | src rows] of d_out)
        self._h_pre: List[Optional[torch.Tensor]] = [None, None]
        self._sflip = 0
        self._h_pouts = [torch.zeros(B, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._pflip = 0
        self._h_fix = [torch.zeros(2 * B, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self.d_fix = torch.zeros(2 * B, dtype=torch.int32, device=self.device)
        # the per-row sampling arrays (models/llama.py SampleArrays image, bmax rows) of a step with a
        # temperature > 0 request, in buffers of their own: d_stage keeps its layout, and a step
        # without such a request never touches them.  Two pinned images, reused two launches later
        self.d_samp = torch.zeros(SAMP_WORDS * B, dtype=torch.int32, device=self.device)
        self._h_samps = [torch.zeros(SAMP_WORDS * B, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._mflip = 0
        # the log-probabilities of a step with a logprobs request ([rows, 1 + 2 * top_n] words per step:
        # chosen logprob | top ids | top logprobs) come back through pinned images next to the token
        # outputs, one pair per launch path, one extra async copy behind the tokens.  A step without
        # such a request never touches them
        self._h_lps = [torch.zeros(B * LP_WORDS, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._h_plps = [torch.zeros(B * LP_WORDS, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        # the penalty / logit_bias image of a step with such a request (models/llama.py LogitEdits):
        # pinned and double-buffered like the prefill metadata, grown on demand (_stage_edits)
        self._h_pen: List[Optional[torch.Tensor]] = [None, None]
        self._nflip = 0
        # guided decoding: the vocabulary's token table and the DFA arena (engine/guided.py GuideTable, created
        # with the first guided request: guides()), and the pinned, double-buffered per-row image of a step
        # with a guided request (_stage_guides).  A step without one touches none of them
        self.tokenizer = tokenizer
        self.guide_states = int(guide_states)
        self.guide_table: Optional[GuideTable] = None
        self.token_table = None
        self._guide_lock = threading.Lock()
        self._h_gds: List[Optional[torch.Tensor]] = [None, None]
        self._gflip = 0
        # ... and the stack image of a step with a row under a stack guide (JSON mode, _stage_guide_stacks)
        self._h_gss: List[Optional[torch.Tensor]] = [None, None]
        self._sflip = 0
        # LoRA (models/lora.py): the per-row adapter slots of a step with at least one adapter row go to the device
        # through two pinned buffers like the sampling image (_stage_adapter); a step without one touches neither
        self._h_ads: List[Optional[torch.Tensor]] = [None, None]
        self._aflip = 0
        # the records of the step read back last (collect / execute), for engine._settle to take
        self.last_logprobs: Optional[StepLogprobs] = None
        self.d_hdr = torch.zeros(HDR, dtype=torch.int32, device=self.device)
        self._h_hdrs = [torch.zeros(HDR, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._hflip = 0
        # the one-shot TP collectives' error word rides back with every step's tokens (a pinned
        # 4-byte copy behind them on the same stream: no extra synchronisation), one slot per launch
        # parity like the token outputs
        self._h_errs = [torch.zeros(2, dtype=torch.int32, pin_memory=pin) for _ in range(4)]
        self._eflip = 0
        # TP decode overlap: rank 0 queues step t+1 (header + staging broadcast + graph) before
        # reading step t back.  Needs collectives that are stream-ordered on the device (RCCL):
        # with a host-synchronous transport (gloo) the step still works, it just does not overlap.
        ov = os.environ.get("KA_TP_OVERLAP", "1")
        self.tp_overlap = tp_size > 1 and (ov == "force" or (ov == "1" and getattr(self.comm, "device_ordered", False)))
        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.graph_pool = None
        self.stats = {"decode_steps": 0, "prefill_steps": 0, "graph_replays": 0, "decode_ms": 0.0,
                      "prefill_ms": 0.0, "prefill_tokens": 0, "persistent_stalls": 0, "sampled_steps": 0,
                      "logprob_steps": 0, "penalty_steps": 0, "guided_steps": 0, "json_steps": 0,
                      "lora_steps": 0}
        # bucket -> the captured graph holds the persistent decode kernel (its error word must be read
        # back on every replay of that graph, whatever model.persistent says now)
        self.graph_persistent: Dict[int, bool] = {}
        # graphs taken out of service while a replay may still be queued (freed by health_check)
        self._retired_graphs: List[object] = []

    # ------------------------------------------------------------------------------------------
    def _view(self, name: str, n: int) -> torch.Tensor:
        o = self._off[name]
        if name == "bt":
            return self.d_stage[o:o + n * self.max_blocks].view(n, self.max_blocks)
        return self.d_stage[o:o + n]

    def _cascade(self, B: int) -> bool:
        return self.cascade_min_b > 0 and B >= self.cascade_min_b and self.device.type == "cuda"

    def _decode_forward(self, B: int, samp: Optional[SampleArrays] = None,
                        adapter: Optional[torch.Tensor] = None) -> None:
        meta = AttnMeta(positions=self._view("pos", B), slot_mapping=self._view("slots", B),
                        block_tables=self._view("bt", B), ctx_lens=self._view("ctx", B),
                        logits_indices=self.d_logits_idx[:B], is_decode=True,
                        shared_blocks=self._view("nsh", 1) if self._cascade(B) else None, adapter=adapter)
        h = self.model.forward(self._view("ids", B), meta, self.k_cache, self.v_cache)
        mask_idx = self._view("mask", B) if self.mask_bits is not None else None
        tok = self.model.sample(h, self.mask_bits, mask_idx, samp)
        self.d_out[:B].copy_(tok)

    def _stage_adapter(self, batch: Batch, rows: int, num_query: Optional[List[int]] = None) -> Optional[torch.Tensor]:
        """The step's LoRA slot per token row on the device (int32 [rows]: a sequence's slot repeated over its
        query rows, -1 for base requests and padding rows), or None when no request of `batch` runs on an
        adapter: that step takes its usual route untouched.  The slot is static per sequence, so chained and
        lookahead steps need no fix-up on the device."""
        slots = [s.params.adapter for s in batch.seqs]
        if all(a is None for a in slots):
            return None
        if self.model.lora is None:
            raise RuntimeError("a request names a LoRA adapter but the engine has none loaded")
        if self.tp_size > 1:
            raise RuntimeError("LoRA adapters are not wired through the TP worker protocol")
        self.stats["lora_steps"] += 1
        per_seq = np.asarray([-1 if a is None else int(a) for a in slots], dtype=np.int32)
        img = np.full(rows, -1, dtype=np.int32)
        if num_query is None:
            img[:len(per_seq)] = per_seq
        else:
            flat = np.repeat(per_seq, np.asarray(num_query, dtype=np.int64))
            img[:flat.shape[0]] = flat
        if self.device.type != "cuda":
            return torch.from_numpy(img)
        k = self._aflip = self._aflip ^ 1
        hb = self._h_ads[k]
        if hb is None or hb.numel() < rows:
            hb = torch.empty(max(rows, 2 * (hb.numel() if hb is not None else 0), self.bmax), dtype=torch.int32,
                             pin_memory=True)
            self._h_ads[k] = hb
        hb.numpy()[:rows] = img
        return hb[:rows].to(self.device, non_blocking=True)

    # ---- steps that need the logits written: a request with temperature > 0, with logprobs, or with
    # penalties / logit_bias ----
    @staticmethod
    def _sampling(batch: Batch) -> bool:
        return any(s.params.temperature > 0 for s in batch.seqs)

    @staticmethod
    def _logprob_n(batch: Batch) -> int:
        """The largest number of alternatives a request of `batch` asks for; -1: none asks for logprobs."""
        return max((int(s.params.logprobs) for s in batch.seqs if s.params.logprobs is not None), default=-1)

    @staticmethod
    def _pack_samp(seqs, h: np.ndarray, cap: int, ahead: int = 0) -> None:
        """Fill a SampleArrays image of `cap` rows.  position: the count that picks the mask row
        (num_generated + ahead), so a token is the same whether its step was chained, scheduled ahead
        or recomputed after a preemption.  Rows of greedy requests and rows past the batch: temperature 0."""
        h[:SAMP_WORDS * cap] = 0
        f = h.view(np.float32)
        f[2 * cap:3 * cap] = 1.0
        sd = h[4 * cap:6 * cap].view(np.uint64)
        for i, s in enumerate(seqs):
            p = s.params
            f[i] = max(0.0, float(p.temperature))
            h[cap + i] = min(max(0, int(p.top_k)), 2 ** 31 - 1)
            f[2 * cap + i] = float(p.top_p)
            h[3 * cap + i] = s.num_generated + ahead
            sd[i] = s.sample_seed

    def _stage_samp(self, batch: Batch, rows: int, ahead: int = 0,
                    pend: Optional[List[int]] = None) -> Optional[SampleArrays]:
        """The step's sampling arrays on the device (`rows` rows: the batch, then greedy padding), or
        None when no request of `batch` samples, asks for logprobs or carries penalties / logit_bias:
        that step takes the greedy path untouched.  With a logprobs request the arrays carry top_n, with
        a penalised one the edit image (`pend`: per batch row the d_out slot of its newest token when
        that is still on the device, else -1), and greedy rows go through ops.sample at temperature 0
        (the masked argmax, bit for bit)."""
        top_n = self._logprob_n(batch)
        penalised = any(s.params.penalised for s in batch.seqs)
        guided = any(s.params.guide is not None for s in batch.seqs)
        if top_n < 0 and not penalised and not guided and not self._sampling(batch):
            return None
        if self.tp_size > 1:
            raise RuntimeError("sampling with temperature > 0, logprobs, penalties and guides are not wired "
                               "through the TP worker protocol")
        self.stats["sampled_steps"] += self._sampling(batch)
        self.stats["logprob_steps"] += top_n >= 0
        self.stats["penalty_steps"] += penalised
        self.stats["guided_steps"] += guided
        samp = self._stage_samp_arrays(batch, rows, ahead)
        samp.top_n = top_n
        if penalised:
            samp.edits = self._stage_edits(batch, rows, pend)
        if guided:
            samp.guide = self._stage_guides(batch, rows, pend)
        return samp

    def guides(self) -> GuideTable:
        """The DFA arena and the token table, built with the first guided request (any thread)."""
        with self._guide_lock:
            if self.guide_table is None:
                if self.tokenizer is None:
                    raise ValueError("guided decoding needs the engine's tokenizer (ModelRunner(tokenizer=...))")
                self.token_table = ops.token_table(self.tokenizer.id_to_bytes, self.tokenizer.eos_ids, self.device)
                self.guide_table = GuideTable(self.guide_states, self.device)
            return self.guide_table

    def _stage_guides(self, batch: Batch, rows: int, pend: Optional[List[int]]) -> GuideArrays:
        """The step's guide image (engine/guided.py pack_guides) -> device without a host sync, through one of
        two pinned buffers like the penalty image.  Guides placed since the last step are uploaded here, on the
        engine's stream: behind every queued step that could still read the range they reuse.  A sequence that
        did not come through engine.submit takes its placement here."""
        table = self.guides()
        for s in batch.seqs:
            if s.params.guide is not None and s.guide_ref is None and not s.finished:
                s.guide_ref = table.acquire(s.params.guide)
        table.flush()
        img = pack_guides(batch.seqs, rows, pend, self.tokenizer)
        if self.device.type != "cuda":
            dimg = torch.from_numpy(img)
        else:
            n = img.shape[0]
            k = self._gflip = self._gflip ^ 1
            hb = self._h_gds[k]
            if hb is None or hb.numel() < n:
                hb = torch.empty(max(n, 4 * self.bmax), dtype=torch.int32, pin_memory=True)
                self._h_gds[k] = hb
            hb.numpy()[:n] = img
            dimg = hb[:n].to(self.device, non_blocking=True)
        arrays = GuideArrays.from_image(dimg, rows, self.token_table, table.trans, table.accept, self.d_out)
        if any(isinstance(s.params.guide, StackGuide) and s.guide_ref is not None for s in batch.seqs):
            self.stats["json_steps"] += 1
            arrays.with_stacks(self._stage_guide_stacks(batch, rows), rows, table.arena_pop)
        return arrays

    def _stage_guide_stacks(self, batch: Batch, rows: int) -> torch.Tensor:
        """The step's stack image (engine/guided.py pack_guide_stacks) -> device, by the route of _stage_guides:
        one of two pinned buffers, no host sync.  Only a step with a row under a stack guide comes here."""
        img = pack_guide_stacks(batch.seqs, rows, self.tokenizer)
        if self.device.type != "cuda":
            return torch.from_numpy(img)
        n = img.shape[0]
        k = self._sflip = self._sflip ^ 1
        hb = self._h_gss[k]
        if hb is None or hb.numel() < n:
            hb = torch.empty(max(n, 10 * self.bmax), dtype=torch.int32, pin_memory=True)
            self._h_gss[k] = hb
        hb.numpy()[:n] = img
        return hb[:n].to(self.device, non_blocking=True)

    def _stage_edits(self, batch: Batch, rows: int, pend: Optional[List[int]]) -> LogitEdits:
        """The step's penalty / logit_bias image (engine/penalties.py pack_edits) -> device without a host
        sync: through one of two pinned buffers, grown on demand (the one refilled here served the
        launch before last, already read back).  The pending tokens are read from d_out on the device."""
        img, E = pack_edits(batch.seqs, rows, pend)
        if self.device.type != "cuda":
            return LogitEdits.from_image(torch.from_numpy(img), rows, E, self.d_out)
        n = img.shape[0]
        k = self._nflip = self._nflip ^ 1
        hb = self._h_pen[k]
        if hb is None or hb.numel() < n:
            hb = torch.empty(max(n, 2 * (hb.numel() if hb is not None else 0), 1 << 14), dtype=torch.int32,
                             pin_memory=True)
            self._h_pen[k] = hb
        hb.numpy()[:n] = img
        return LogitEdits.from_image(hb[:n].to(self.device, non_blocking=True), rows, E, self.d_out)

    def _stage_samp_arrays(self, batch: Batch, rows: int, ahead: int) -> SampleArrays:
        if rows > self.bmax:   # a synchronous step larger than the buffers (execute)
            img = np.zeros(SAMP_WORDS * rows, dtype=np.int32)
            self._pack_samp(batch.seqs, img, rows, ahead)
            return SampleArrays.from_image(torch.from_numpy(img).to(self.device), rows, rows)
        hb = self._h_samps[self._mflip]
        self._mflip ^= 1
        self._pack_samp(batch.seqs, hb.numpy(), self.bmax, ahead)
        self.d_samp.copy_(hb, non_blocking=True)
        return SampleArrays.from_image(self.d_samp, self.bmax, rows)

    def _copy_logprobs(self, samp: Optional[SampleArrays], rows: int, bufs: List[torch.Tensor], k: int):
        """Queue the readback of the step's log-probabilities (the first `rows` rows) behind its tokens:
        packed on the device into [rows, 1 + 2 * top_n] words, then one async copy into pinned image
        bufs[k].  -> (image, top_n), or (None, 0) for a step without a logprobs request."""
        if samp is None or samp.logprobs is None:
            return None, 0
        lp, tid, tlp = samp.logprobs
        n = samp.top_n
        img = torch.cat([lp[:rows, None].view(torch.int32), tid[:rows], tlp[:rows].view(torch.int32)], dim=1)
        h = bufs[k][:rows * (1 + 2 * n)].view(rows, 1 + 2 * n)
        h.copy_(img, non_blocking=True)
        return h, n

    @staticmethod
    def _host_logprobs(samp: Optional[SampleArrays], rows: int) -> Optional[StepLogprobs]:
        """The synchronous path's records, straight from the device tensors."""
        if samp is None or samp.logprobs is None:
            return None
        lp, tid, tlp = (t[:rows].cpu().numpy() for t in samp.logprobs)
        return StepLogprobs(lp, tid, tlp)

    @staticmethod
    def _read_logprobs(h: Optional[torch.Tensor], n: int) -> Optional[StepLogprobs]:
        """A pinned image whose copy has completed -> records (copied out: the image is reused)."""
        if h is None:
            return None
        a = h.numpy()
        return StepLogprobs(a[:, 0].copy().view(np.float32), a[:, 1:1 + n].copy(),
                            a[:, 1 + n:1 + 2 * n].copy().view(np.float32))

    def _attention_consumer(self, ctx: int = 128):
        """fn(qkv, M): decode_attention_rope over M synthetic sequences of `ctx` cached tokens in
        layer 0's cache (tuning runs before serving: the KV written here is never read), for
        tune_gemm_plan to time QKV with; None where that kernel cannot read this cache (16-token blocks)."""
        m, bs = self.model, self.block_size
        if bs != 16:
            return None
        nb = (ctx + bs - 1) // bs
        memo = {}

        def consume(qkv, M):
            if M not in memo:
                bt = (torch.arange(M * nb, dtype=torch.int32, device=self.device) % self.num_blocks).view(M, nb)
                pos = torch.full((M,), ctx - 1, dtype=torch.int32, device=self.device)
                slots = (bt[:, -1] * bs + (ctx - 1) % bs).to(torch.int32)
                lens = torch.full((M,), ctx, dtype=torch.int32, device=self.device)
                memo[M] = (pos, slots, bt.contiguous(), lens)
            pos, slots, bt, lens = memo[M]
            return ops.decode_attention_rope(qkv, pos, m.cos_sin, slots, self.k_cache[0], self.v_cache[0], bt, lens,
                                             m.hq, m.hkv, m.D, m.scale)
        return consume

    @torch.inference_mode()
    def capture_graphs(self, autotune: bool = True) -> float:
        """Capture one decode graph per bucket (largest first, sharing a memory pool)."""
        if not self.use_graphs:
            return 0.0
        t0 = time.perf_counter()
        if self.device.type == "cuda":
            ops.gemm_big_ws(self.device)   # allocated (and zeroed) outside any capture
        if autotune:
            self.plans = tune_engine(self.model, self.buckets, self.mask_bits, self._attention_consumer())
        self.h_np[:] = 0
        o = self._off
        for name in ("slots",):
            self.h_np[o[name]:o[name] + self.bmax] = -1
        self.h_np[o["mask"]:o["mask"] + self.bmax] = -1
        self.d_stage.copy_(self.h_stage)
        stream = torch.cuda.Stream(self.device)
        stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(stream):
            for B in reversed(self.buckets):
                self._decode_forward(B)  # warm-up (hipBLASLt heuristics, allocator)
        torch.cuda.current_stream(self.device).wait_stream(stream)
        torch.cuda.synchronize(self.device)
        for B in reversed(self.buckets):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.graph_pool):
                self._decode_forward(B)
            if self.graph_pool is None:
                self.graph_pool = g.pool()
            self.graphs[B] = g
            self.graph_persistent[B] = self.model.persistent_ok(B)
        torch.cuda.synchronize(self.device)
        return time.perf_counter() - t0

    # ------------------------------------------------------------------------------------------
    def _slot(self, table: List[int], pos: int) -> int:
        return table[pos // self.block_size] * self.block_size + pos % self.block_size

    def _pack_decode(self, batch: Batch, Bp: int, h: Optional[np.ndarray] = None, ahead: int = 0) -> None:
        """Fill the decode staging image.  ahead = 1: for the step after the one in flight (its token
        is not appended yet; ids then come from the device, launch_decode_async)."""
        h = self.h_np if h is None else h
        o, mb = self._off, self.max_blocks
        B = len(batch.seqs)
        for i, s in enumerate(batch.seqs):
            if not s.block_table:   # a freed (finished) sequence: its slots would alias block 0
                raise RuntimeError(f"decode row {i} (seq {s.seq_id}) has no KV blocks")
            L = s.total_len + ahead
            pos = L - 1
            h[o["ids"] + i] = s.all_ids[-1] if not ahead else 0
            h[o["pos"] + i] = pos
            h[o["slots"] + i] = self._slot(s.block_table, pos)
            h[o["ctx"] + i] = L
            h[o["mask"] + i] = mask_index_for(s.num_generated + ahead, s.params.safe_decode)
            row = o["bt"] + i * mb
            n = len(s.block_table)
            h[row:row + n] = s.block_table
        if Bp > B:  # padding rows: no cache write, empty context
            for name, val in (("ids", 0), ("pos", 0), ("slots", -1), ("ctx", 0), ("mask", -1)):
                h[o[name] + B:o[name] + Bp] = val
        h[o["nsh"]] = self._shared_prefix_blocks(batch, h, ahead) if self._cascade(Bp) else 0

    def _shared_prefix_blocks(self, batch: Batch, h: np.ndarray, ahead: int) -> int:
        """Leading block-table entries that every row shares, counting only blocks full of cached
        tokens (the new token's block is each row's own)."""
        o, mb, B = self._off, self.max_blocks, len(batch.seqs)
        lim = min((s.total_len + ahead - 1) // self.block_size for s in batch.seqs)
        return shared_prefix_len(h[o["bt"]:o["bt"] + B * mb].reshape(B, mb), lim)

    def can_overlap(self, B: int) -> bool:
        """A decode step of B rows can be queued before the previous one is read back.
        (on CPU the "async" launch simply runs synchronously: same code path, testable)"""
        return (self.tp_size == 1 or self.tp_overlap) and B <= self.bmax

    def can_overlap_prefill(self, B: int) -> bool:
        return (self.tp_size == 1 or self.tp_overlap) and B <= self.bmax

    def can_lookahead(self) -> bool:
        """Steps can be scheduled and queued ahead of the in-flight step's readback.  With TP, rank 0
        applies the placeholder fixups on the device BEFORE the staging broadcast (every rank samples
        the same tokens into its d_out, but only rank 0 knows the fixup list), so the other ranks
        receive final inputs; needs stream-ordered collectives (tp_overlap) to actually overlap."""
        return self.tp_size == 1 or self.tp_overlap

    @torch.inference_mode()
    def launch_decode_async(self, batch: Batch, chained: bool = False, fix: Optional[List[tuple]] = None):
        """Queue one decode step without waiting for it.  chained: `batch` is the step after the one
        in flight (same sequences, same row order): its input ids are copied on the device from the
        previous step's sampled tokens (with TP, on rank 0 before the staging broadcast, so the other
        ranks receive them; every rank samples the same token).  fix: (row, src) pairs of rows whose
        input is a PLACEHOLDER: their ids are the in-flight step's sampled tokens d_out[src] (a step
        scheduled ahead, engine._lookahead_step).  Returns a handle for `collect`."""
        B = len(batch.seqs)
        i = bisect.bisect_left(self.buckets, B)
        Bp = self.buckets[i] if i < len(self.buckets) else B
        t0 = time.perf_counter()
        k = self._flip
        self._flip ^= 1
        hs, ho = self._h_stages[k], self._h_outs[k]
        self._pack_decode(batch, Bp, hs.numpy(), ahead=1 if chained else 0)
        n_copy = self._off["bt"] + Bp * self.max_blocks
        self._bcast_header_async(KIND_DECODE, Bp, n_copy)
        self.d_stage[:n_copy].copy_(hs[:n_copy], non_blocking=True)
        if chained:
            o = self._off["ids"]
            self.d_stage[o:o + B].copy_(self.d_out[:B])
        if fix:
            nf = len(fix)
            hf = self._h_fix[k]
            hf.numpy()[:2 * nf] = np.asarray(fix, dtype=np.int32).T.reshape(-1)
            self.d_fix[:2 * nf].copy_(hf[:2 * nf], non_blocking=True)
            o = self._off["ids"]
            self.d_stage[o:o + Bp].index_copy_(0, self.d_fix[:nf].long(),
                                               self.d_out.index_select(0, self.d_fix[nf:2 * nf].long()))
        # rows whose newest output token is still in d_out (not in output_ids, or there as a PLACEHOLDER):
        # what a penalised row's counts are still missing
        pend = None
        if chained:
            pend = list(range(B))
        elif fix:
            pend = [-1] * B
            for row, src in fix:
                pend[row] = src
        samp = self._stage_samp(batch, Bp, ahead=1 if chained else 0, pend=pend)
        adapter = self._stage_adapter(batch, Bp)
        self._launch_decode(Bp, n_copy, samp, adapter)
        ho[:B].copy_(self.d_out[:B], non_blocking=True)
        lh, ln = self._copy_logprobs(samp, B, self._h_lps, k)
        # a sampled step ran eagerly beside the bucket's graph: the model's current setting decides
        # whether it launched the persistent kernel, not what the graph was captured with
        eager = samp is not None or adapter is not None
        eh = self._copy_err(persistent=self._persistent_step(Bp) if not eager
                            else adapter is None and self.model.persistent_ok(Bp))
        ev = None
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        return StepHandle(ev, ho, B, t0, err_host=eh, lp_host=lh, lp_n=ln)

    @torch.inference_mode()
    def launch_prefill_async(self, batch: Batch):
        """Queue a prefill or mixed step without waiting for its tokens (at most `bmax` rows; with TP,
        rank 0 broadcasts the header and the fixed-up metadata, stream-ordered):
        the sampled tokens are also left in `d_out`, in batch row order, so the next step can be
        queued right behind it with its inputs taken on the device (`launch_decode_async(chained=
        True)` for the same rows, or the PLACEHOLDER fixups of a step scheduled ahead).  Rows whose
        input is a PLACEHOLDER (this batch was scheduled ahead of the in-flight step's readback) get
        it from `d_out` before the forward.  Returns a handle for `collect`."""
        t0 = time.perf_counter()
        host, nf = self._pack_prefill(batch, pad=True, with_fix=True)
        T, S, max_q, nc = self.padded_tokens(batch.num_tokens), len(batch.seqs), max(batch.num_query), len(batch.copies)
        nd = S - len(batch.prefill_seqs) if self.split_mixed_attention else 0
        buf = self._stage_prefill(host)
        if nf:   # trailing [dst positions | src rows]
            n = buf.shape[0]
            buf[:T].index_copy_(0, buf[n - 2 * nf:n - nf].long(), self.d_out.index_select(0, buf[n - nf:].long()))
            buf = buf[:n - 2 * nf]
        if self.tp_size > 1:   # the other ranks get the fixed-up metadata (worker_loop KIND_PREFILL)
            self._bcast_header_async(KIND_PREFILL, T, S, max_q, buf.shape[0], nc, nd, batch.num_tokens)
            self.comm.broadcast(buf, src=0)
        self.model.mark_layer = max(0, self.cfg.num_layers - self.lookahead_layers)
        self.model.mark_event = None
        # the decode rows of a mixed step scheduled ahead: the same rows _pack_prefill fixed up
        pend = [s.ph_row if s.ph_row is not None and s.num_computed + nq == s.total_len else -1
                for s, nq in zip(batch.seqs, batch.num_query)] if nf else None
        samp = self._stage_samp(batch, S, pend=pend)
        adapter = self._stage_adapter(batch, T, batch.num_query)
        try:
            tok = self._run_prefill(buf, T, S, max_q, nc, nd, batch.num_tokens, samp, adapter)
        finally:
            self.model.mark_layer = -1
        progress, self.model.mark_event = self.model.mark_event, None
        self.d_out[:S].copy_(tok)
        k = self._pflip
        ho = self._h_pouts[k]
        self._pflip ^= 1
        ho[:S].copy_(tok, non_blocking=True)
        lh, ln = self._copy_logprobs(samp, S, self._h_plps, k)
        eh = self._copy_err()
        ev = None
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        return StepHandle(ev, ho, S, t0, prefill_tokens=T, progress=progress, err_host=eh, lp_host=lh, lp_n=ln)

    def _stage_prefill(self, host: np.ndarray) -> torch.Tensor:
        """Packed prefill metadata -> device without a host sync: through one of two pinned buffers
        (grown on demand; the one being refilled served the launch before last, already read back)."""
        if self.device.type != "cuda":
            return torch.from_numpy(host)
        n = host.shape[0]
        k = self._sflip = self._sflip ^ 1
        hb = self._h_pre[k]
        if hb is None or hb.numel() < n:
            hb = torch.empty(max(n, 2 * (hb.numel() if hb is not None else 0), 1 << 16), dtype=torch.int32,
                             pin_memory=True)
            self._h_pre[k] = hb
        hb.numpy()[:n] = host
        return hb[:n].to(self.device, non_blocking=True)

    @torch.inference_mode()
    def health_check(self) -> None:
        """Raise if the device no longer answers: a tiny kernel through the stream and a sync."""
        probe = self.d_out[:1] + 0
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        int(probe[0].item())
        # nothing queued before the synchronize can still be replaying a retired graph
        self._retired_graphs.clear()

    def _err_word(self) -> Optional[torch.Tensor]:
        car = getattr(self.comm, "custom_ar", None)
        return car.state[2:3] if car is not None else None

    def _persistent_step(self, Bp: int) -> bool:
        """The decode step of bucket Bp runs the persistent kernel (its error word is read back): the
        captured graph decides when there is one (a graph captured with the kernel keeps launching it
        after model.persistent is turned off), the model's current setting otherwise."""
        if Bp in self.graphs:
            return self.graph_persistent.get(Bp, False)
        return self.model.persistent_ok(Bp)

    def _copy_err(self, persistent: bool = False) -> Optional[torch.Tensor]:
        """Queue the error word's readback behind the step just launched: [one-shot collectives,
        persistent decode kernel] (None when the step has neither)."""
        src = self._err_word()
        psrc = self.model.persistent_err_word() if persistent else None
        if src is None and psrc is None:
            return None
        h = self._h_errs[self._eflip]
        self._eflip = (self._eflip + 1) % len(self._h_errs)
        h.zero_()
        if src is not None:
            h[0:1].copy_(src, non_blocking=True)
        if psrc is not None:
            h[1:2].copy_(psrc, non_blocking=True)
        return h

    def _check_err(self, h: Optional[torch.Tensor]) -> None:
        if h is None:
            return
        if int(h[0]):
            raise CollectiveTimeout("one-shot TP collective: a peer never arrived (spin timeout); "
                                    "the step's results are stale")
        if int(h[1]):
            self.model.persistent = False   # the chain from now on: co-residency cannot be relied on
            # a graph captured with the persistent kernel would keep replaying it: take those graphs
            # out of service (their buckets run eagerly, the kernel chain, from the next step on).  The
            # engine may already have queued a chained step that replays one of them, so the graph
            # objects are only retired here; health_check() frees them after a device synchronize
            # (destroying a hipGraphExec with a launch still pending is not defined)
            for b in [b for b, p in self.graph_persistent.items() if p]:
                g = self.graphs.pop(b, None)
                if g is not None:
                    self._retired_graphs.append(g)
                self.graph_persistent.pop(b, None)
            self.stats["persistent_stalls"] += 1
            logger.error("persistent decode kernel: a grid wait ran out; batch-1 decode falls back to "
                         "the kernel chain (stall #%d)", self.stats["persistent_stalls"])
            raise PersistentStall("persistent decode: a workgroup never ran (grid wait timeout); "
                                  "the step's results are stale")

    def collect(self, handle: "StepHandle") -> List[int]:
        """Wait for a queued step and return its tokens.  The step's log-probability records (None
        without a logprobs request) are left in `last_logprobs` for engine._settle."""
        ev, ho, B, t0 = handle.event, handle.host_out, handle.rows, handle.t0
        self.last_logprobs = None
        if handle.prefill_tokens:   # launch_prefill_async
            if ev is not None:
                ev.synchronize()
            self.last_logprobs = self._read_logprobs(handle.lp_host, handle.lp_n)
            now = time.perf_counter()
            self.stats["prefill_steps"] += 1
            self.stats["prefill_tokens"] += handle.prefill_tokens
            self.stats["prefill_ms"] += (now - t0) * 1e3
            self._last_collect = now
            self._check_err(handle.err_host)
            return ho[:B].tolist()
        if ev is not None:
            ev.synchronize()
        self._check_err(handle.err_host)
        self.last_logprobs = self._read_logprobs(handle.lp_host, handle.lp_n)
        now = time.perf_counter()
        # wall time attributed to this step: from its launch (or the previous collect, if later)
        self.stats["decode_ms"] += (now - max(t0, getattr(self, "_last_collect", t0))) * 1e3
        self._last_collect = now
        self.stats["decode_steps"] += 1
        return ho[:B].tolist()

    def _launch_decode(self, Bp: int, n_copy: int, samp: Optional[SampleArrays] = None,
                       adapter: Optional[torch.Tensor] = None) -> None:
        if self.tp_size > 1:
            self.comm.broadcast(self.d_stage[:n_copy], src=0)
        # the captured graphs end in the greedy sampler and hold the base model's route: a step with a sampling
        # request or with LoRA rows runs eagerly
        eager = samp is not None or adapter is not None
        g = self.graphs.get(Bp) if not eager else None
        if eager:
            self._decode_forward(Bp, samp, adapter)
        elif g is not None:
            g.replay()
            self.stats["graph_replays"] += 1
        else:
            self._decode_forward(Bp)

    def padded_tokens(self, T: int) -> int:
        """Prefill steps of >= 1024 tokens run padded to a multiple of KA_PREFILL_PAD (256): hipBLASLt
        is up to ~10% faster per token on whole 256-row tiles (scripts/bench_prefill_gemm.py: M=4000
        1.31 PFLOP/s vs M=4096 1.45).  Padding rows write no KV (slot -1) and are never sampled."""
        q = self.prefill_pad
        return T if q <= 1 or T < self.prefill_pad_min else (T + q - 1) // q * q

    def _pack_prefill(self, batch: Batch, pad: bool = False, with_fix: bool = False):
        """Packed step metadata [ids | pos | slots | q_starts | ctx | mask | logits idx | block tables |
        copies (src, dst) | fixups (dst, src)].  with_fix: also returns the number of PLACEHOLDER
        fixups (flat id position, in-flight row) appended at the end (their ids are packed as the
        placeholder and replaced on the device)."""
        S = len(batch.seqs)
        T = self.padded_tokens(batch.num_tokens) if pad else batch.num_tokens
        mb = self.max_blocks
        nc = len(batch.copies)
        fix = []
        if with_fix:
            q0 = 0
            for s, nq in zip(batch.seqs, batch.num_query):
                # a placeholder is always the sequence's last token; the row covers it if it ends there
                if s.ph_row is not None and s.num_computed + nq == s.total_len:
                    fix.append((q0 + nq - 1, s.ph_row))
                q0 += nq
        nf = len(fix)
        buf = np.zeros(3 * T + (S + 1) + 3 * S + S * mb + 2 * nc + 2 * nf, dtype=np.int32)
        if nf:
            fx = np.asarray(fix, dtype=np.int32)
            buf[len(buf) - 2 * nf:len(buf) - nf] = fx[:, 0]
            buf[len(buf) - nf:] = fx[:, 1]
        if nc:   # [src... | dst...] block-copy list (sub-block prefix reuse), before the fixups
            cp = np.asarray(batch.copies, dtype=np.int32)
            e = len(buf) - 2 * nf
            buf[e - 2 * nc:e - nc] = cp[:, 0]
            buf[e - nc:e] = cp[:, 1]
        ids, pos, slots = buf[:T], buf[T:2 * T], buf[2 * T:3 * T]
        slots[batch.num_tokens:] = -1          # padding rows (if any): no cache write
        o = 3 * T
        q_starts = buf[o:o + S + 1]; o += S + 1
        ctx = buf[o:o + S]; o += S
        mask = buf[o:o + S]; o += S
        lidx = buf[o:o + S]; o += S
        bt = buf[o:o + S * mb].reshape(S, mb)
        # one Python pass collects per-sequence scalars, token slices and tables; the per-token
        # arrays are then built with a handful of vectorised numpy ops (was ~10 numpy calls per
        # sequence: ~2.7 ms of GPU-idle host time for a 256-request prefill)
        nqs = np.asarray(batch.num_query, dtype=np.int64)
        tot = np.empty(S, dtype=np.int64)
        toks: list = []
        for i, (s, nq) in enumerate(zip(batch.seqs, batch.num_query)):
            start = s.num_computed               # query = all_ids[start:n] (a chunk may end early)
            n = start + nq
            tot[i] = n
            ng = len(s.output_ids) - s.n_forced
            lp = len(s.prompt_ids)
            if start >= lp:                      # decode row (mixed step): generated tokens only
                toks.extend(s.output_ids[s.n_forced + start - lp:s.n_forced + n - lp])
            else:
                toks.extend(s.prompt_ids[start:min(n, lp)])
                if n > lp:
                    toks.extend(s.output_ids[s.n_forced:s.n_forced + n - lp])
            tbl = s.block_table
            if not tbl:   # a freed (finished) sequence: its slots would alias block 0
                raise RuntimeError(f"prefill row {i} (seq {s.seq_id}) has no KV blocks")
            bt[i, :len(tbl)] = tbl
            mask[i] = mask_index_for(ng, s.params.safe_decode)
        n_real = int(nqs.sum())
        ends = np.cumsum(nqs)
        q_starts[0] = 0
        q_starts[1:] = ends
        ctx[:] = tot
        lidx[:] = ends - 1
        ids[:n_real] = toks
        seq_of = np.repeat(np.arange(S), nqs)
        p = np.arange(n_real, dtype=np.int64) - np.repeat(ends - nqs, nqs) + np.repeat(tot - nqs, nqs)
        pos[:n_real] = p
        bs = self.block_size
        slots[:n_real] = bt[seq_of, p // bs] * bs + p % bs
        return (buf, nf) if with_fix else buf

    def _run_prefill(self, buf: torch.Tensor, T: int, S: int, max_q: int, nc: int = 0, nd: int = 0,
                     t_real: int = 0, samp: Optional[SampleArrays] = None,
                     adapter: Optional[torch.Tensor] = None) -> torch.Tensor:
        mb = self.max_blocks
        if nc:
            n = buf.shape[0]
            ops.kv_block_copy(self.k_cache, self.v_cache, buf[n - 2 * nc:n - nc], buf[n - nc:])
        ids, pos, slots = buf[:T], buf[T:2 * T], buf[2 * T:3 * T]
        o = 3 * T
        q_starts = buf[o:o + S + 1]; o += S + 1
        ctx = buf[o:o + S]; o += S
        mask = buf[o:o + S]; o += S
        lidx = buf[o:o + S].long(); o += S
        bt = buf[o:o + S * mb].view(S, mb)
        meta = AttnMeta(positions=pos, slot_mapping=slots, block_tables=bt, ctx_lens=ctx, logits_indices=lidx,
                        is_decode=False, q_starts=q_starts, max_q_len=max_q, num_decode=nd,
                        num_tokens=t_real or T, adapter=adapter)
        h = self.model.forward(ids, meta, self.k_cache, self.v_cache)
        return self.model.sample(h, self.mask_bits, mask if self.mask_bits is not None else None, samp)

    # ------------------------------------------------------------------------------------------
    def _bcast_header(self, kind: int, a: int = 0, b: int = 0, c: int = 0, d: int = 0, e: int = 0,
                      f: int = 0, g: int = 0) -> None:
        if self.tp_size == 1:
            return
        self.d_hdr.copy_(torch.tensor([kind, a, b, c, d, e, f, g], dtype=torch.int32))
        self.comm.broadcast(self.d_hdr, src=0)

    def _bcast_header_async(self, kind: int, *vals: int) -> None:
        """The step header from pinned memory (the copy stays asynchronous on the stream); two
        buffers: the one refilled here served the launch before last, which has been read back."""
        if self.tp_size == 1:
            return
        hh = self._h_hdrs[self._hflip]
        self._hflip ^= 1
        h = hh.numpy()
        h[:] = 0
        h[0] = kind
        h[1:1 + len(vals)] = vals
        self.d_hdr.copy_(hh, non_blocking=True)
        self.comm.broadcast(self.d_hdr, src=0)

    @torch.inference_mode()
    def execute(self, batch: Batch) -> List[int]:
        """Run one step for `batch` on every TP rank; returns the sampled token per sequence."""
        B = len(batch.seqs)
        if B == 0:
            return []
        t0 = time.perf_counter()
        self.last_logprobs = None
        if batch.is_decode and B <= self.bmax:
            i = bisect.bisect_left(self.buckets, B)
            # pad to the bucket even when running eagerly: identical shapes -> identical GEMM plans
            # and kernels as the captured graphs (graph replay == eager, token for token)
            Bp = self.buckets[i] if i < len(self.buckets) else B
            self._pack_decode(batch, Bp)
            n_copy = self._off["bt"] + Bp * self.max_blocks
            self._bcast_header(KIND_DECODE, Bp, n_copy)
            self.d_stage[:n_copy].copy_(self.h_stage[:n_copy], non_blocking=True)
            samp = self._stage_samp(batch, Bp)
            self._launch_decode(Bp, n_copy, samp, self._stage_adapter(batch, Bp))
            self.h_out[:B].copy_(self.d_out[:B], non_blocking=True)
            eh = self._copy_err()
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()
            self._check_err(eh)
            out = self.h_out[:B].tolist()
            self.last_logprobs = self._host_logprobs(samp, B)
            self.stats["decode_steps"] += 1
            self.stats["decode_ms"] += (time.perf_counter() - t0) * 1e3
            return out
        host = self._pack_prefill(batch, pad=True)
        T, S, max_q, nc = self.padded_tokens(batch.num_tokens), B, max(batch.num_query), len(batch.copies)
        nd = B - len(batch.prefill_seqs) if self.split_mixed_attention else 0
        self._bcast_header(KIND_PREFILL, T, S, max_q, host.shape[0], nc, nd, batch.num_tokens)
        buf = torch.from_numpy(host).to(self.device, non_blocking=False)
        if self.tp_size > 1:
            self.comm.broadcast(buf, src=0)
        samp = self._stage_samp(batch, S)
        tok = self._run_prefill(buf, T, S, max_q, nc, nd, batch.num_tokens, samp,
                                self._stage_adapter(batch, T, batch.num_query))
        eh = self._copy_err()
        out = tok.cpu().tolist()
        self._check_err(eh)
        self.last_logprobs = self._host_logprobs(samp, S)
        self.stats["prefill_steps"] += 1
        self.stats["prefill_tokens"] += T
        self.stats["prefill_ms"] += (time.perf_counter() - t0) * 1e3
        return out

    @torch.inference_mode()
    def worker_loop(self) -> None:
        """Non-driver TP ranks: mirror every step of rank 0 until it broadcasts STOP.  A worker whose
        one-shot collective timed out is out of step with the group: it raises (the process exits,
        its heartbeat stops, rank 0's watchdog marks the engine unhealthy).  The error word of a step
        is read after the next header arrives (that readback synchronises the stream anyway)."""
        pending = None
        while True:
            self.comm.broadcast(self.d_hdr, src=0)
            kind, a, b, c, d, e, f, g = self.d_hdr[:8].tolist()
            self._check_err(pending)
            if kind == KIND_STOP:
                return
            if kind == KIND_DECODE:
                self._launch_decode(a, b)
            elif kind == KIND_PREFILL:
                buf = torch.empty(d, dtype=torch.int32, device=self.device)
                self.comm.broadcast(buf, src=0)
                self._run_prefill(buf, a, b, c, e, f, g)
            pending = self._copy_err()

    def stop_workers(self) -> None:
        self._bcast_header(KIND_STOP)
