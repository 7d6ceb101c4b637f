"""Plain-PyTorch fp32 reference implementations of every engine op.

These define the semantics the HIP kernels (`csrc/*.hip`) must match; the GPU numerics tests
compare kernel output against them, and CPU-only runs (tests, no GPU) execute the engine through
them.  Layouts are documented in `csrc/elementwise.hip` / `csrc/attention.hip`.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """y = x @ w.T computed in fp32 (the reference for every projection), returned in x's dtype."""
    return torch.nn.functional.linear(x.float(), w.float()).to(x.dtype)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    if residual is not None:
        r = (x.float() + residual.float()).to(x.dtype)
        residual.copy_(r)
        x = r
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(x.dtype)


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, device=None) -> torch.Tensor:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def rope_kv_write(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, hq: int, hkv: int, d: int):
    T = qkv.shape[0]
    half = d // 2
    q = qkv[:, : hq * d].view(T, hq, d).float()
    k = qkv[:, hq * d: (hq + hkv) * d].view(T, hkv, d).float()
    v = qkv[:, (hq + hkv) * d:].view(T, hkv, d)
    cs = cos_sin[positions.long()]
    cos, sin = cs[:, None, :half], cs[:, None, half:]

    def rot(x):
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)

    q_out = rot(q).to(qkv.dtype)
    k_rot = rot(k).to(qkv.dtype)
    bs = k_cache.shape[2]
    slots = slot_mapping.long()
    valid = slots >= 0
    if valid.any():
        s = slots[valid]
        blk, off = s // bs, s % bs
        k_cache[blk, :, off, :] = k_rot[valid].to(k_cache.dtype)
        v_cache[blk, :, :, off] = v[valid].to(v_cache.dtype)
    return q_out


def _gather_kv(k_cache, v_cache, table_row, ctx: int):
    bs = k_cache.shape[2]
    nb = (ctx + bs - 1) // bs
    blocks = table_row[:nb].long()
    k = k_cache[blocks]                       # [nb, Hkv, bs, D]
    v = v_cache[blocks].transpose(-1, -2)     # [nb, Hkv, bs, D]
    k = k.permute(1, 0, 2, 3).reshape(k.shape[1], nb * bs, -1)[:, :ctx]
    v = v.permute(1, 0, 2, 3).reshape(v.shape[1], nb * bs, -1)[:, :ctx]
    return k.float(), v.float()               # [Hkv, ctx, D]


def attention_prefill(q, k_cache, v_cache, block_tables, q_starts, ctx_lens, scale: float):
    T, hq, d = q.shape
    hkv = k_cache.shape[1]
    G = hq // hkv
    out = torch.zeros_like(q)
    qs = q_starts.tolist()
    cl = ctx_lens.tolist()
    for s in range(len(cl)):
        q0, q1, ctx = qs[s], qs[s + 1], cl[s]
        qlen = q1 - q0
        if qlen == 0 or ctx == 0:      # ctx 0 = padding row of a bucketed decode batch
            continue
        k, v = _gather_kv(k_cache, v_cache, block_tables[s], ctx)
        k = k.repeat_interleave(G, dim=0)
        v = v.repeat_interleave(G, dim=0)
        qq = q[q0:q1].float().transpose(0, 1)            # [Hq, qlen, D]
        sc = torch.matmul(qq, k.transpose(-1, -2)) * scale  # [Hq, qlen, ctx]
        qpos = torch.arange(ctx - qlen, ctx, device=q.device)
        kpos = torch.arange(ctx, device=q.device)
        sc = sc.masked_fill(kpos[None, None, :] > qpos[None, :, None], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[q0:q1] = torch.matmul(p, v).transpose(0, 1).to(q.dtype)
    return out


def attention_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale: float):
    B = q.shape[0]
    starts = torch.arange(B + 1, dtype=torch.int32, device=q.device)
    return attention_prefill(q, k_cache, v_cache, block_tables, starts, ctx_lens, scale)


def silu_mul(gu: torch.Tensor) -> torch.Tensor:
    i = gu.shape[-1] // 2
    g, u = gu[..., :i].float(), gu[..., i:].float()
    return (F.silu(g) * u).to(gu.dtype)


def embedding(ids: torch.Tensor, table: torch.Tensor, vocab_offset: int = 0) -> torch.Tensor:
    local = ids.long() - vocab_offset
    valid = (local >= 0) & (local < table.shape[0])
    out = table[local.clamp(0, table.shape[0] - 1)]
    return out * valid[:, None].to(out.dtype)


def masked_argmax(logits, mask_bits, mask_idx, vocab_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    lf = logits.float().clone()
    V = lf.shape[1]
    if mask_bits is not None and mask_idx is not None:
        gid = torch.arange(V, device=logits.device) + vocab_offset
        words = mask_bits[:, gid // 32].long()                      # [M, V]
        allowed = ((words >> (gid % 32)) & 1).bool()
        mi = mask_idx.long().to(logits.device)
        rows = allowed[mi.clamp(min=0)] | (mi < 0)[:, None]
        lf = lf.masked_fill(~rows, float("-inf"))
    idx = torch.argmax(lf, dim=-1)   # documented: first index of the maximum (= kernel tie-break)
    val = lf.gather(1, idx[:, None]).squeeze(1)
    return (idx + vocab_offset).to(torch.int32), val


def moe_topk(router_logits: torch.Tensor, k: int):
    p = torch.softmax(router_logits.float(), dim=-1)
    w, ids = torch.topk(p, k, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    return w, ids.to(torch.int32)


def argmax_combine(vals: torch.Tensor, idxs: torch.Tensor) -> torch.Tensor:
    """[ranks, S] (value, global id) pairs -> [S] int32: the largest value, the lowest id on ties."""
    v = vals.float()
    best = v.max(dim=0, keepdim=True).values
    big = torch.iinfo(torch.int32).max
    cand = torch.where(v == best, idxs.to(torch.int64), torch.full_like(idxs, big, dtype=torch.int64))
    return cand.min(dim=0).values.to(torch.int32)


# ---- seeded temperature / top-k / top-p sampling (csrc/sampling_stochastic.hip) ----
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z):
    """splitmix64's finaliser on numpy uint64 arrays (arithmetic modulo 2^64)."""
    import numpy as np
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_noise_u(seed: int, position: int, gids) -> "np.ndarray":
    """u in (0, 1) per global token id, float64 holding the exact fp32 value the kernel computes:
    key = mix(seed + (position + 1) * G); z = mix(key + (gid + 1) * G); u = (2 * (z >> 41) + 1) * 2^-24."""
    import numpy as np
    g = np.uint64(_GOLDEN)
    s = np.asarray([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    key = _mix64(s + np.asarray([int(position) + 1], dtype=np.uint64) * g)
    z = _mix64(key + (np.asarray(gids, dtype=np.uint64) + np.uint64(1)) * g)
    return (2.0 * (z >> np.uint64(41)).astype(np.float64) + 1.0) * 2.0 ** -24


def _bf16_key(x: torch.Tensor) -> torch.Tensor:
    """Order-preserving 16-bit key (int64) of bf16 values: larger value <=> larger key; -0 counts as +0."""
    b = x.to(torch.bfloat16).contiguous().view(torch.int16).long() & 0xFFFF
    b = torch.where(b == 0x8000, torch.zeros_like(b), b)
    return torch.where((b & 0x8000) != 0, b ^ 0xFFFF, b | 0x8000)


def _bf16_key_value(k: torch.Tensor) -> torch.Tensor:
    b = torch.where((k & 0x8000) != 0, k & 0x7FFF, k ^ 0xFFFF)
    b = torch.where(b >= 0x8000, b - 0x10000, b)
    return b.to(torch.int16).view(torch.bfloat16).float()


def sample(logits, mask_bits, mask_idx, temperature, top_k, top_p, seed, position, vocab_offset: int = 0,
           return_cut: bool = False, dtype=torch.float32, return_margins: bool = False):
    """Gumbel-max sampling per row among the tokens mask row `mask_idx[r]` allows (-1 = all):
    temperature 0 = `masked_argmax`; top_k = k keeps the logits >= the min(k, allowed)-th largest
    (ties stay); top_p = p then keeps the logits >= the first value (walking the distinct values
    downwards) at which the mass of exp((l - max) / T) reaches p x the total; the token is the argmax
    of l / T - log(-log(u)) over the kept set (lowest id on ties), u = `sample_noise_u`.
    -> (idx int32, val fp32) [+ (cut fp32, kept int32) with return_cut: the cut-off logit (-inf
    without an active cut) and the number of tokens at or above it] [+ (gap, p_lo, p_hi) with
    return_margins, in `dtype`: best minus second-best score (inf for temperature 0 or one kept
    token), and how far p lies above the cumulative mass share just before the cut value / below the
    share including it (inf without top-p)].  dtype: of the scores and masses (float64: ground truth)."""
    idx, val = masked_argmax(logits, mask_bits, mask_idx, vocab_offset)
    R, V = logits.shape
    dev = logits.device
    val = val.float().clone()
    cut = torch.full((R,), float("-inf"), dtype=torch.float32, device=dev)
    kept = torch.zeros(R, dtype=torch.int32, device=dev)
    gap = torch.full((R,), float("inf"), dtype=dtype, device=dev)
    p_lo = torch.full((R,), float("inf"), dtype=dtype, device=dev)
    p_hi = torch.full((R,), float("inf"), dtype=dtype, device=dev)
    gid = torch.arange(V, device=dev) + vocab_offset
    if mask_bits is not None and mask_idx is not None:
        words = mask_bits[:, gid // 32].long()
        allowed_rows = ((words >> (gid % 32)) & 1).bool()
    temps = temperature.float().cpu().tolist()
    ks, ps = top_k.cpu().tolist(), top_p.float().cpu().tolist()
    seeds, poss = seed.cpu().tolist(), position.cpu().tolist()
    gid_np = gid.cpu().numpy()
    for r in range(R):
        T = temps[r]
        mi = int(mask_idx[r]) if (mask_bits is not None and mask_idx is not None) else -1
        allowed = allowed_rows[mi] if mi >= 0 else torch.ones(V, dtype=torch.bool, device=dev)
        n_allowed = int(allowed.sum())
        kept[r] = n_allowed
        if not T > 0 or n_allowed == 0:
            continue
        l = logits[r].float()
        keep = allowed
        if ks[r] > 0 or ps[r] < 1:
            la = l[allowed]
            k = min(ks[r], n_allowed) if ks[r] > 0 else n_allowed
            tau = torch.topk(la, k).values[-1]
            if ps[r] < 1:
                lk = la[la >= tau]
                # a bf16 logit has 65,536 possible values: one mass bin per value, by its ordered key
                key = _bf16_key(lk)
                w = torch.exp((lk.to(dtype) - lk.max().to(dtype)) / T)
                mass = torch.bincount(key, weights=w, minlength=65536).to(dtype)
                vals = torch.bincount(key, minlength=65536).nonzero().squeeze(1).flip(0)   # distinct, downwards
                cum = torch.cumsum(mass[vals], 0)
                total = cum[-1]
                j = int((cum >= ps[r] * total).nonzero()[0])
                tau = _bf16_key_value(vals[j])
                p_hi[r] = cum[j] / total - ps[r]
                p_lo[r] = ps[r] - (cum[j - 1] / total if j > 0 else 0.0)
            cut[r] = tau
            keep = allowed & (l >= tau)
            kept[r] = int(keep.sum())
        u = torch.from_numpy(sample_noise_u(seeds[r], poss[r], gid_np)).to(dev)
        g = -torch.log(-torch.log(u.to(dtype)))
        score = (l.to(dtype) / T + g).masked_fill(~keep, float("-inf"))
        i = int(torch.argmax(score))   # first index of the maximum
        idx[r] = i + vocab_offset
        val[r] = score[i]
        if int(kept[r]) > 1:
            gap[r] = score[i] - torch.topk(score, 2).values[1]
    out = (idx, val)
    if return_cut:
        out += (cut, kept)
    if return_margins:
        out += (gap, p_lo, p_hi)
    return out


# ---- per-token log-probabilities (csrc/logprobs.hip) ----
def token_logprobs(logits, mask_bits, mask_idx, token, top_n: int, vocab_offset: int = 0,
                   return_probe: bool = False, dtype=torch.float32):
    """Log-probability of `token[r]` (global id) and the `top_n` most likely tokens per row among the
    tokens mask row `mask_idx[r]` allows (-1 = all), A:
        m = max over A of l;  w = exp(l - m);  mass = sum over A of trunc(w * 2^40) (an integer);
        S = mass * 2^-40;  logprob(i) = (l_i - m) - log(S), -inf outside A or outside the vocab slice.
    This is the model's distribution under the mask BEFORE temperature / top-k / top-p / seed, which
    shape the draw only.  A weight below 2^-40 counts as zero.  The top list is ordered by (exact bf16
    value descending, global id ascending): a prefix of the top-20 list; entries past |A| are id -1,
    -inf.  dtype: of the weights, the logarithm and the subtractions (float64: ground truth).
    -> (lp [R], top_id int32 [R, top_n], top_lp [R, top_n]) [+ (max fp32, count int32, mass int64) with
    return_probe]; lp and top_lp in `dtype`."""
    R, V = logits.shape
    dev = logits.device
    lp = torch.full((R,), float("-inf"), dtype=dtype, device=dev)
    top_id = torch.full((R, top_n), -1, dtype=torch.int32, device=dev)
    top_lp = torch.full((R, top_n), float("-inf"), dtype=dtype, device=dev)
    mx = torch.full((R,), float("-inf"), dtype=torch.float32, device=dev)
    cnt = torch.zeros(R, dtype=torch.int32, device=dev)
    mass = torch.zeros(R, dtype=torch.int64, device=dev)
    gid = torch.arange(V, device=dev) + vocab_offset
    masked = mask_bits is not None and mask_idx is not None
    if masked:
        words = mask_bits[:, gid // 32].long()
        allowed_rows = ((words >> (gid % 32)) & 1).bool()
    toks = token.cpu().tolist()
    for r in range(R):
        mi = int(mask_idx[r]) if masked else -1
        allowed = allowed_rows[mi] if mi >= 0 else torch.ones(V, dtype=torch.bool, device=dev)
        ids = allowed.nonzero().squeeze(1)
        cnt[r] = ids.numel()
        if ids.numel() == 0:
            continue
        la = logits[r].float()[ids]
        m = la.max()
        mx[r] = m + 0.0   # -0 counts as +0
        d = la.to(dtype) - m.to(dtype)
        wi = torch.trunc(torch.exp(d) * 2.0 ** 40).to(torch.int64)
        mass[r] = wi.sum()
        log_s = torch.log(mass[r].to(dtype) * 2.0 ** -40)
        all_lp = d - log_s
        i = toks[r] - vocab_offset
        if 0 <= i < V and bool(allowed[i]):
            lp[r] = (logits[r, i].float().to(dtype) - m.to(dtype)) - log_s
        if top_n:
            # everything at or above the n-th largest value, in id order, then a stable sort by value:
            # ties keep the lowest id first
            pool = (la >= torch.topk(la, min(top_n, la.numel())).values[-1]).nonzero().squeeze(1)
            order = pool[torch.sort(la[pool], descending=True, stable=True).indices[:top_n]]
            n = order.numel()
            top_id[r, :n] = (ids[order] + vocab_offset).to(torch.int32)
            top_lp[r, :n] = all_lp[order]
    out = (lp, top_id, top_lp)
    if return_probe:
        out += (mx, cnt, mass)
    return out


# ---- penalties and logit_bias (csrc/logit_adjust.hip) ----
PROMPT_BIT = 0x80000000   # bit 31 of an entry's cnt word: the token occurs in the prompt


def _pending(pend_src, tokens, r: int) -> int:
    """Global id of row r's pending token (tokens[pend_src[r]]), -1 without one."""
    if pend_src is None or tokens is None:
        return -1
    ps = int(pend_src[r])
    return int(tokens[ps]) if 0 <= ps < tokens.numel() else -1


def _row_skipped(n_entries: int, pend: bool, pres: float, freq: float, rep: float) -> bool:
    return n_entries == 0 and (not pend or (pres == 0.0 and freq == 0.0 and rep == 1.0))


def logit_adjust(logits, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src=None,
                 tokens=None, vocab_offset: int = 0, save: bool = False):
    """presence / frequency / repetition penalties and logit_bias, in place on bf16 `logits` [R, V]: THE
    definition (csrc/logit_adjust.hip and the engine match it bit for bit).

    Row r owns the entries row_start[r] .. row_start[r + 1]: `ent_id` (global token id, distinct within a
    row), `ent_cnt` (int32: bits 0-30 = c, the token's occurrences in the sequence's output so far, the
    jump-forward prefix included; bit 31 = it occurs in the prompt) and `ent_bias` (fp32, 0 without a
    logit_bias entry); `presence`, `frequency`, `repetition` are fp32 [R].  With seen = c > 0 or the
    prompt bit, every operation in fp32 and rounded separately, in this order:
        x = float(logit)
        if seen and repetition != 1:  x = x / repetition if x > 0 else x * repetition
        x = x - frequency * float(c);  x = x - (presence if c > 0 else 0);  x = x + bias
        logit = bf16 round-to-nearest-even(x)
    Tokens without an entry do not change; an entry outside [vocab_offset, vocab_offset + V) is skipped.
    An adjustment below half a bf16 ulp of the logit therefore leaves it as it is, and a touched -0
    comes out as +0 (x + 0), which every consumer treats alike.
    pend_src int32 [R] with tokens int32: pend_src[r] >= 0 says the row's newest output token is
    tokens[pend_src[r]] and the entries do not count it: it gets c + 1 and seen, as one more entry
    (c = 1, no prompt bit, bias 0) when no entry has its id.  A row without entries is left alone when
    it has no pending token or its three parameters are neutral.
    save: -> bf16 [R + entries], the original patterns (slot r: the pending token of row r when it had
    no entry; slot R + e: entry e; slots never written hold 0) for logit_restore; else -> None."""
    R, V = logits.shape
    E = int(ent_id.numel())
    saved = torch.zeros(R + E, dtype=logits.dtype, device=logits.device) if save else None
    rs = row_start.tolist()
    for r in range(R):
        e0, e1 = max(0, rs[r]), min(E, rs[r + 1])
        pres, freq, rep = presence[r].float(), frequency[r].float(), repetition[r].float()
        pend = _pending(pend_src, tokens, r)
        if _row_skipped(max(0, e1 - e0), pend >= 0, float(pres), float(freq), float(rep)):
            continue
        ids = ent_id[e0:e1].long()
        word = ent_cnt[e0:e1].long() & 0xFFFFFFFF
        c = word & (PROMPT_BIT - 1)
        prompt = (word & PROMPT_BIT) != 0
        bias = ent_bias[e0:e1].float()
        slot = torch.arange(e0, e1, device=logits.device) + R
        if pend >= 0:
            hit = ids == pend
            if bool(hit.any()):
                c = c + hit.long()
            else:
                ids = torch.cat([ids, ids.new_tensor([pend])])
                c = torch.cat([c, c.new_tensor([1])])
                prompt = torch.cat([prompt, prompt.new_tensor([False])])
                bias = torch.cat([bias, bias.new_zeros(1)])
                slot = torch.cat([slot, slot.new_tensor([r])])
        li = ids - vocab_offset
        ok = (li >= 0) & (li < V)
        li, c, prompt, bias, slot = li[ok], c[ok], prompt[ok], bias[ok], slot[ok]
        raw = logits[r, li]
        if save:
            saved[slot] = raw
        x = raw.float()
        if float(rep) != 1.0:
            x = torch.where(prompt | (c > 0), torch.where(x > 0, x / rep, x * rep), x)
        x = x - freq * c.float()
        x = x - torch.where(c > 0, pres, torch.zeros_like(pres))
        x = x + bias
        logits[r, li] = x.to(logits.dtype)
    return saved


def logit_restore(logits, row_start, ent_id, presence, frequency, repetition, pend_src, tokens, saved,
                  vocab_offset: int = 0) -> None:
    """Write back what logit_adjust(save=True) saved, from the same image and the same `tokens`."""
    R, V = logits.shape
    E = int(ent_id.numel())
    rs = row_start.tolist()
    for r in range(R):
        e0, e1 = max(0, rs[r]), min(E, rs[r + 1])
        pend = _pending(pend_src, tokens, r)
        if _row_skipped(max(0, e1 - e0), pend >= 0, float(presence[r]), float(frequency[r]), float(repetition[r])):
            continue
        ids = ent_id[e0:e1].long()
        slot = torch.arange(e0, e1, device=logits.device) + R
        if pend >= 0 and not bool((ids == pend).any()):
            ids = torch.cat([ids, ids.new_tensor([pend])])
            slot = torch.cat([slot, slot.new_tensor([r])])
        li = ids - vocab_offset
        ok = (li >= 0) & (li < V)
        logits[r, li[ok]] = saved[slot[ok]]


def guide_mask(table, arena_trans, arena_accept, row_base, row_nstates, row_state, pend_src, tokens, base_bits,
               base_idx):
    """The definition of ops.guide_mask (csrc/guide_mask.hip): per guided row the vocabulary bitmask of the
    tokens that keep the row's DFA alive, intersected with the row's SAFE_DECODE mask.

    table: ops.TokenTable (byte strings of the V tokens, EOS ids).  arena_trans int16 [G, 256] (uint16
    patterns, 0xFFFF = dead, local state numbers), arena_accept uint8 [G]; per row: row_base (arena base, < 0
    = not guided), row_nstates, row_state (local, outside [0, nstates) = dead), pend_src (None or int32: a
    value in [0, n_tokens) names tokens[pend_src], the row's newest token, walked first: an EOS id leaves the
    state, an id outside [0, V) or a token without bytes kills it).  base_bits int32 [n_static, words] or
    None with base_idx int32 [R] (< 0 = no base row).
    -> bits int32 [n_static + R, words] (rows 0..n_static-1 = base_bits, row n_static + r = batch row r, zero
    for a row that is not guided; bit t set when (t is an EOS id and the state is live and accepting, or t
    has bytes and they never reach dead) and the base row allows t; an empty row gets eos_ids[0]),
    idx int32 [R] (n_static + r for a guided row, else base_idx[r] or -1), state_after int32 [R] (-1 = dead
    or not guided).  Vectorised by byte position over the tokens still alive."""
    import numpy as np
    V, words = table.vocab, (table.vocab + 31) // 32
    R = int(row_base.shape[0])
    G = int(arena_trans.shape[0])
    tr = arena_trans.cpu().numpy().view(np.uint16)
    acc = arena_accept.cpu().numpy()
    base = row_base.cpu().numpy()
    nst = row_nstates.cpu().numpy()
    st = row_state.cpu().numpy()
    ps = pend_src.cpu().numpy() if pend_src is not None else None
    toks = tokens.cpu().numpy() if tokens is not None else np.zeros(0, dtype=np.int32)
    bb = base_bits.cpu().numpy().view(np.uint32) if base_bits is not None else None
    bi = base_idx.cpu().numpy() if base_idx is not None and bb is not None else None
    n_static = bb.shape[0] if bb is not None else 0
    bits = np.zeros((n_static + R, words), dtype=np.uint32)
    if n_static:
        bits[:n_static] = bb
    idx = np.full(R, -1, dtype=np.int32)
    after = np.full(R, -1, dtype=np.int32)
    mat, lens, eos = table.mat, table.lens, table.eos
    has_bytes = np.flatnonzero(lens > 0)
    for r in range(R):
        if base[r] < 0:
            if bi is not None:
                idx[r] = bi[r]
            continue
        idx[r] = n_static + r
        b0 = int(base[r])
        n = max(0, min(int(nst[r]), G - b0))     # states of this guide that lie inside the arena
        s = int(st[r]) if 0 <= int(st[r]) < n else -1

        def step(states, byts):
            nxt = tr[b0 + states, byts].astype(np.int64)
            return np.where(nxt < n, nxt, -1)

        if ps is not None and 0 <= int(ps[r]) < toks.shape[0]:
            t = int(toks[int(ps[r])])
            if 0 <= t < V and eos[t]:
                pass
            elif not 0 <= t < V or lens[t] == 0:
                s = -1
            else:
                for b in mat[t, :lens[t]]:
                    s = int(step(np.asarray([s]), np.asarray([b]))[0]) if s >= 0 else -1
        after[r] = s
        allowed = np.zeros(V, dtype=bool)
        if s >= 0:
            alive = has_bytes
            cur = np.full(alive.shape[0], s, dtype=np.int64)
            pos = 0
            done = []
            while alive.size:
                ended = lens[alive] == pos
                done.append(alive[ended])
                alive, cur = alive[~ended], cur[~ended]
                if not alive.size:
                    break
                cur = step(cur, mat[alive, pos])
                keep = cur >= 0
                alive, cur = alive[keep], cur[keep]
                pos += 1
            if done:
                allowed[np.concatenate(done)] = True
            if acc[b0 + s]:
                allowed |= eos
        if bi is not None and bi[r] >= 0:
            row = bb[bi[r]]
            allowed &= ((row[np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1).astype(bool)
        if not allowed.any():
            allowed[table.eos_ids[0]] = True
        padded = np.zeros(words * 32, dtype=bool)
        padded[:V] = allowed
        bits[n_static + r] = np.packbits(padded, bitorder="little").view(np.uint32)
    dev = row_base.device
    return (torch.from_numpy(bits.view(np.int32)).to(dev), torch.from_numpy(idx).to(dev),
            torch.from_numpy(after).to(dev))


def _stack_words(stack):
    """uint32 [8]: the symbols, bottom first, symbol i in bits 4 (i mod 8) of word i / 8."""
    import numpy as np
    w = np.zeros(8, dtype=np.uint32)
    for i, y in enumerate(stack):
        w[i >> 3] |= np.uint32(int(y) << (4 * (i & 7)))
    return w


def guide_mask_stack(table, arena_trans, arena_accept, arena_pop, row_base, row_nstates, row_state, row_kind,
                     row_depth, row_stack, pend_src, tokens, base_bits, base_idx):
    """The definition of ops.guide_mask_stack (csrc/guide_stack.hip): guide_mask for a step with rows under a
    stack guide (engine/guided.py StackGuide, JSON mode).

    As guide_mask, plus arena_pop int16 [G, 16] (row `base` of a guide's range: its pop_to, uint16 patterns),
    row_kind int32 [R] (0: a DFA row, exactly guide_mask's entry semantics; 1: a stack row), row_depth int32 [R]
    and row_stack int32 [R, 8] (64 four-bit symbols, bottom first, symbol i in bits 4 (i mod 8) of word i / 8).
    A stack row whose depth is outside 0..64 or that holds a symbol 0 or 15 below its depth is dead.

    An entry e of a stack row, in a state s inside [0, n): 0xFFFF dead.  Bit 15 set: a pop; push bits 11-14
    that are not 0, or an empty stack: dead; else the top symbol y is taken and the next state is pop_to[y]
    (not below n: dead).  Bit 15 clear: the next state is bits 0-10 (not below n: dead); push bits y that are
    not 0 push y: y = 15, a stack that already holds 64 symbols, or 16 symbols that THIS token pushed and that
    are still on the stack: dead.  Every token starts from the row's stack after the pending token.
    -> (bits, idx, state_after) as guide_mask, depth_after int32 [R], stack_after int32 [R, 8]: the row after
    its pending token (what the mask was built from); 0 for a row that is dead, not guided or of kind 0."""
    import numpy as np
    V, words = table.vocab, (table.vocab + 31) // 32
    R = int(row_base.shape[0])
    G = int(arena_trans.shape[0])
    tr = arena_trans.cpu().numpy().view(np.uint16)
    acc = arena_accept.cpu().numpy()
    apop = arena_pop.cpu().numpy().view(np.uint16)
    base = row_base.cpu().numpy()
    nst = row_nstates.cpu().numpy()
    st = row_state.cpu().numpy()
    kind = row_kind.cpu().numpy()
    dep = row_depth.cpu().numpy()
    stk = row_stack.cpu().numpy().view(np.uint32).reshape(R, 8)
    ps = pend_src.cpu().numpy() if pend_src is not None else None
    toks = tokens.cpu().numpy() if tokens is not None else np.zeros(0, dtype=np.int32)
    bb = base_bits.cpu().numpy().view(np.uint32) if base_bits is not None else None
    bi = base_idx.cpu().numpy() if base_idx is not None and bb is not None else None
    n_static = bb.shape[0] if bb is not None else 0
    bits = np.zeros((n_static + R, words), dtype=np.uint32)
    if n_static:
        bits[:n_static] = bb
    idx = np.full(R, -1, dtype=np.int32)
    after = np.full(R, -1, dtype=np.int32)
    depth_after = np.zeros(R, dtype=np.int32)
    stack_after = np.zeros((R, 8), dtype=np.uint32)
    mat, lens, eos = table.mat, table.lens, table.eos
    has_bytes = np.flatnonzero(lens > 0)
    for r in range(R):
        if base[r] < 0:
            if bi is not None:
                idx[r] = bi[r]
            continue
        idx[r] = n_static + r
        b0 = int(base[r])
        n = max(0, min(int(nst[r]), G - b0))     # states of this guide that lie inside the arena
        s = int(st[r]) if 0 <= int(st[r]) < n else -1
        stacked = int(kind[r]) == 1
        popto = apop[b0].astype(np.int64) if stacked and b0 < G else np.full(16, 0xFFFF, dtype=np.int64)
        row = []                                 # the row's stack, bottom first
        if stacked:
            d = int(dep[r])
            if 0 <= d <= 64:
                row = [(int(stk[r, i >> 3]) >> (4 * (i & 7))) & 15 for i in range(d)]
            if not 0 <= d <= 64 or any(y in (0, 15) for y in row):
                s, row = -1, []

        # one byte for every token of `cur` (states), `reg` (the symbols each token pushed, newest in the low
        # four bits), `cnt` (how many of them) and `cons` (symbols each took from the row's stack `rowsym`)
        def step(cur, reg, cnt, cons, byts, rowsym):
            e = tr[b0 + cur, byts].astype(np.int64)
            if not stacked:
                return np.where(e < n, e, -1), reg, cnt, cons
            y = (e >> 11) & 15
            is_pop = (e & 0x8000) != 0
            tgt = e & 0x7FF
            depth = len(rowsym) - cons + cnt
            go = ~is_pop & (tgt < n) & (y != 15)
            push = go & (y > 0)
            go &= ~push | ((depth < 64) & (cnt < 16))
            push &= go
            pop = is_pop & (y == 0) & (depth > 0)
            from_reg = pop & (cnt > 0)
            from_row = pop & (cnt == 0)
            padded = np.asarray(list(rowsym) + [0], dtype=np.int64)
            sym = np.where(from_reg, (reg & np.uint64(15)).astype(np.int64),
                           padded[np.clip(len(rowsym) - 1 - cons, -1, len(rowsym) - 1)])
            sym = np.where(pop, sym, 0)
            to = popto[sym]
            pop &= (sym >= 1) & (sym <= 14) & (to < n)
            from_reg &= pop
            from_row &= pop
            nxt = np.where(go, tgt, np.where(pop, to, -1))
            reg = np.where(push, (reg << np.uint64(4)) | y.astype(np.uint64), np.where(from_reg, reg >> np.uint64(4), reg))
            return nxt, reg, cnt + push - from_reg, cons + from_row

        if ps is not None and 0 <= int(ps[r]) < toks.shape[0]:
            t = int(toks[int(ps[r])])
            if 0 <= t < V and eos[t]:
                pass
            elif not 0 <= t < V or lens[t] == 0:
                s = -1
            elif s >= 0:
                cur, reg = np.asarray([s], dtype=np.int64), np.zeros(1, dtype=np.uint64)
                cnt, cons = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
                for b in mat[t, :lens[t]]:
                    cur, reg, cnt, cons = step(cur, reg, cnt, cons, np.asarray([b]), row)
                    if cur[0] < 0:
                        break
                s = int(cur[0])
                if s >= 0 and stacked:           # the token's own symbols go on top of what it left of the row's
                    own = [(int(reg[0]) >> (4 * i)) & 15 for i in range(int(cnt[0]))][::-1]
                    row = row[:len(row) - int(cons[0])] + own
        if s < 0:
            row = []
        after[r] = s
        if stacked:
            depth_after[r] = len(row)
            stack_after[r] = _stack_words(row)
        allowed = np.zeros(V, dtype=bool)
        if s >= 0:
            alive = has_bytes
            m = alive.shape[0]
            cur, reg = np.full(m, s, dtype=np.int64), np.zeros(m, dtype=np.uint64)
            cnt, cons = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
            pos = 0
            done = []
            while alive.size:
                ended = lens[alive] == pos
                done.append(alive[ended])
                keep = ~ended
                alive, cur, reg, cnt, cons = alive[keep], cur[keep], reg[keep], cnt[keep], cons[keep]
                if not alive.size:
                    break
                cur, reg, cnt, cons = step(cur, reg, cnt, cons, mat[alive, pos], row)
                keep = cur >= 0
                alive, cur, reg, cnt, cons = alive[keep], cur[keep], reg[keep], cnt[keep], cons[keep]
                pos += 1
            if done:
                allowed[np.concatenate(done)] = True
            if acc[b0 + s]:
                allowed |= eos
        if bi is not None and bi[r] >= 0:
            brow = bb[bi[r]]
            allowed &= ((brow[np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1).astype(bool)
        if not allowed.any():
            allowed[table.eos_ids[0]] = True
        padded = np.zeros(words * 32, dtype=bool)
        padded[:V] = allowed
        bits[n_static + r] = np.packbits(padded, bitorder="little").view(np.uint32)
    dev = row_base.device
    return (torch.from_numpy(bits.view(np.int32)).to(dev), torch.from_numpy(idx).to(dev),
            torch.from_numpy(after).to(dev), torch.from_numpy(depth_after).to(dev),
            torch.from_numpy(stack_after.view(np.int32)).to(dev))


def lora_add(y, x, row_adapter, A, B, scale, seg):
    """Per-row LoRA (csrc/lora.hip): in place y[i] += scale[a, s] * (x[i] A[a, s]^T) B[a, seg[s]:seg[s + 1]]^T
    for a = row_adapter[i] >= 0.  y [T, N], x [T, K], row_adapter int32 [T] (-1: the row has no adapter),
    A [n_adapters, S, R, K], B [n_adapters, N, R], scale fp32 [n_adapters, S], seg the S + 1 segment boundaries
    of N.  t = x A^T is accumulated in fp32 and rounded to bf16 (part of the definition: the expand step runs on
    the bf16 MFMA), t B^T is accumulated in fp32, and y is rounded once.  Rows of -1 and segments of scale 0 keep
    their bits."""
    seg = [int(v) for v in seg]
    ra = row_adapter.long().cpu()
    sc_h = scale.float().cpu()
    for a in sorted(set(ra.tolist())):
        if a < 0 or a >= A.shape[0]:
            continue
        rows = (ra == a).nonzero().flatten().to(y.device)
        xf = x.index_select(0, rows).float()
        for s in range(len(seg) - 1):
            sc = float(sc_h[a, s])
            if sc == 0.0:
                continue
            t = (xf @ A[a, s].float().T).to(torch.bfloat16).float()
            d = t @ B[a, seg[s]:seg[s + 1]].float().T
            cur = y[:, seg[s]:seg[s + 1]].index_select(0, rows).float()
            y[:, seg[s]:seg[s + 1]].index_copy_(0, rows, (cur + sc * d).to(y.dtype))
    return y
