"""Host bookkeeping of the penalty / logit_bias fields: what ops.logit_adjust (csrc/logit_adjust.hip) is fed.

Per penalised sequence a `PenaltyState` keeps the entries of its row of the CSR image: one per token
that can change, i.e. every token of the output (c > 0), every logit_bias id and, only when
repetition_penalty != 1 (nothing else reads the prompt bit), every distinct id of the prompt.  The
static part (bias ids, the prompt's up to 8192 distinct ids) is built once; each step only counts the
output tokens that became final since the last one, so a step costs the new tokens plus three array
copies per row.  The counts come from `output_ids` (the jump-forward prefix included), never from the
prompt, and a recompute preemption leaves both lists as they are: the state stays valid across it.
(`Sequence.__post_init__` appends the jump-forward prefix to `prompt_ids` as well as to `output_ids`, so its
tokens carry the prompt bit and a count: they are `seen` either way, and only `output_ids` feeds `c`.)

A trailing PLACEHOLDER (a token still on the device, engine._lookahead_step) is not counted: the runner
names its device slot in `pend_src` and the kernel adds it.
"""
from __future__ import annotations

from typing import List, Optional, Sequence as Seq

import numpy as np

from .sequence import PLACEHOLDER, SamplingParams, Sequence

PROMPT_BIT = np.uint32(0x80000000)
MAX_BIAS_ENTRIES = 300


def validate(p: SamplingParams, vocab_size: int, tp_size: int) -> None:
    """Raise ValueError (HTTP 400 / 422 upstream) naming the field that is out of range."""
    if not -2.0 <= float(p.presence_penalty) <= 2.0:
        raise ValueError("presence_penalty must be in -2..2")
    if not -2.0 <= float(p.frequency_penalty) <= 2.0:
        raise ValueError("frequency_penalty must be in -2..2")
    if not 0.0 < float(p.repetition_penalty) <= 2.0:
        raise ValueError("repetition_penalty must be in (0, 2]")
    bias = p.logit_bias or {}
    if len(bias) > MAX_BIAS_ENTRIES:
        raise ValueError(f"logit_bias holds {len(bias)} entries; at most {MAX_BIAS_ENTRIES} are accepted")
    for t, b in bias.items():
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < vocab_size:
            raise ValueError(f"logit_bias token id {t!r} is outside the vocabulary [0, {vocab_size})")
        if not -100.0 <= float(b) <= 100.0:   # a NaN fails both comparisons
            raise ValueError(f"logit_bias value {b!r} for token {t} must be in -100..100")
    if p.penalised and tp_size > 1:
        # the logits are vocab-parallel and the worker protocol does not carry the image
        raise ValueError("presence_penalty / frequency_penalty / repetition_penalty / logit_bias are not supported "
                         "with tensor parallelism (TP > 1)")


class PenaltyState:
    """One sequence's entries: ids (int32), cnt (uint32: bits 0-30 = c, bit 31 = occurs in the prompt) and
    bias (fp32), the first `n` of each array; `counted` output tokens are in the counts."""

    def __init__(self, seq: Sequence):
        p = seq.params
        bias = {int(t): float(b) for t, b in (p.logit_bias or {}).items()}
        self.prompt = set(seq.prompt_ids)
        pa = np.unique(np.asarray(seq.prompt_ids, dtype=np.int64))
        ba = np.asarray(sorted(bias), dtype=np.int64)
        first = np.union1d(pa, ba) if p.repetition_penalty != 1 else ba
        n = self.n = int(first.shape[0])
        # every output token can add one entry (max_new_tokens of them, after the jump-forward prefix)
        cap = n + seq.n_forced + int(p.max_new_tokens) + 1
        self.ids = np.zeros(cap, dtype=np.int32)
        self.cnt = np.zeros(cap, dtype=np.uint32)
        self.bias = np.zeros(cap, dtype=np.float32)
        self.ids[:n] = first
        self.cnt[:n] = np.where(np.isin(first, pa), PROMPT_BIT, np.uint32(0))
        self.bias[np.searchsorted(first, ba)] = [bias[t] for t in ba.tolist()]
        self.index = dict(zip(first.tolist(), range(n)))
        self.counted = 0

    def update(self, seq: Sequence) -> None:
        """Count the output tokens that became final since the last call."""
        out = seq.output_ids
        n = len(out) - (1 if out and out[-1] == PLACEHOLDER else 0)
        for t in out[self.counted:n]:
            if t < 0:
                raise RuntimeError(f"seq {seq.seq_id}: an unsettled token inside output_ids")
            i = self.index.get(t)
            if i is None:
                i = self.index[t] = self.n
                if i >= self.ids.shape[0]:   # more outputs than max_new_tokens promised: grow
                    for name in ("ids", "cnt", "bias"):
                        a = getattr(self, name)
                        setattr(self, name, np.concatenate([a, np.zeros(max(64, a.shape[0]), dtype=a.dtype)]))
                self.ids[i] = t
                self.cnt[i] = PROMPT_BIT if t in self.prompt else 0
                self.bias[i] = 0.0
                self.n += 1
            self.cnt[i] += 1
        self.counted = max(self.counted, n)


def state_of(seq: Sequence) -> PenaltyState:
    st = seq.penalty_state
    if st is None:
        st = seq.penalty_state = PenaltyState(seq)
    st.update(seq)
    return st


def pack_edits(seqs: Seq[Sequence], rows: int, pend: Optional[List[int]] = None):
    """-> (int32 image, entries) of models/llama.py LogitEdits for a step of `rows` rows (the batch, then
    padding): [row_start (rows + 1) | presence | frequency | repetition | pend_src (rows each) | ids | cnts |
    biases (entries each)].  Rows of requests without penalties and padding rows: empty segments, neutral
    parameters, no pending token.  pend: per batch row, the d_out slot of the row's newest, still
    uncounted output token, or -1 (None: no row has one)."""
    states = [state_of(s) if s.params.penalised else None for s in seqs]
    E = sum(st.n for st in states if st is not None)
    img = np.zeros(5 * rows + 1 + 3 * E, dtype=np.int32)
    f = img.view(np.float32)
    o = rows + 1
    f[o + 2 * rows:o + 3 * rows] = 1.0      # repetition
    img[o + 3 * rows:o + 4 * rows] = -1     # pend_src
    ent = o + 4 * rows
    e = 0
    for i, (s, st) in enumerate(zip(seqs, states)):
        img[i] = e
        if st is None:
            continue
        p = s.params
        f[o + i] = p.presence_penalty
        f[o + rows + i] = p.frequency_penalty
        f[o + 2 * rows + i] = p.repetition_penalty
        if pend is not None:
            img[o + 3 * rows + i] = pend[i]
        n = st.n
        img[ent + e:ent + e + n] = st.ids[:n]
        img[ent + E + e:ent + E + e + n] = st.cnt[:n].view(np.int32)
        f[ent + 2 * E + e:ent + 2 * E + e + n] = st.bias[:n]
        e += n
    img[len(seqs):rows + 1] = e
    return img, E
