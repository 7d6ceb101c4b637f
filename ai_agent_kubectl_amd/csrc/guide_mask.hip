// Guided decoding (`guided_regex` / `guided_choice` of /v1/chat/completions): every step, turn each guided
// row's (DFA, state) into the row's vocabulary bitmask by walking every token's bytes through the DFA.
// Semantics: ops/reference.py `guide_mask`.  Everything is integer.
//
// Token table (ops.token_table), one 16-byte record per token, read as one 128-bit load:
//   byte 0      bits 0-4: the number of bytes, 0..15 (0 = the token spells nothing), or 31 = longer than 15;
//               bit 7: the token is an EOS id
//   bytes 1-15  the token's bytes (up to 15)
//   a longer token: bytes 4-7 = offset into the overflow pool, bytes 8-11 = its length there
// DFA arena (engine/guided.py GuideTable): uint16 [arena_states, 256] and uint8 accept flags.  A row's guide
// occupies states [base, base + nstates); its entries are local state numbers, 0xFFFF (or anything that is
// not below nstates) = dead.  Every lookup is guarded: a state is used only while 0 <= s < min(nstates,
// arena_states - base), a token id only inside [0, vocab), an overflow run only inside the pool.
//
// Grid (vocabulary tile, row), GM_NT threads, GM_UN rounds of one token per lane.  The records of all the
// workgroup's tokens and the SAFE_DECODE words they will be intersected with are loaded first; then the
// row's pending token (pend_src: the newest output token, still on the device) is walked, uniform over
// the workgroup; then the tokens are walked byte position by byte position, the GM_UN rounds side by side,
// so a lane has GM_UN independent 2-byte lookups in flight per position (docs/ARCHITECTURE.md, latency-bound
// kernels), and a wave leaves the walk once none of its tokens is alive and unfinished.  The 64-lane
// ballot of "allowed" is two finished mask words: no atomics, no read-modify-write.  A row that is not
// guided gets zero words and idx = its SAFE_DECODE row.  A second kernel, one workgroup per row, gives a
// row whose mask came out empty (a dead state, or nothing left under the SAFE_DECODE mask) the bit of
// eos_ids[0], so the sampler always has a candidate.
#include "common.h"

namespace {

constexpr int GM_NT = 256;
constexpr int GM_UN = 4;
constexpr int GM_TILE = GM_NT * GM_UN;   // tokens per workgroup
constexpr uint32_t GM_EOS = 0x80u;
constexpr uint32_t GM_LONG = 31u;
constexpr int GM_INLINE = 15;

// byte k (1..15) of a record
KA_DEV uint32_t rec_byte(const uint4& r, int k) {
  const uint32_t w = k < 4 ? r.x : k < 8 ? r.y : k < 12 ? r.z : r.w;
  return (w >> (8 * (k & 3))) & 0xffu;
}

// one step from s (any value) under byte b: -1 when s is not a state of the guide or the entry is dead.
// n >= 1 (callers check): the load of a dead lane reads state 0's row and is discarded
KA_DEV int gm_step(const uint16_t* __restrict__ tr, int n, int s, uint32_t b) {
  const bool live = s >= 0 && s < n;
  const uint32_t nx = tr[(size_t)(live ? s : 0) * 256 + b];
  return (live && nx < (uint32_t)n) ? (int)nx : -1;
}

KA_DEV int gm_walk_long(const uint16_t* __restrict__ tr, int n, int s, const uint8_t* __restrict__ ovf,
                        int ovf_bytes, uint32_t off, uint32_t len) {
  if (len == 0u || off > (uint32_t)ovf_bytes || len > (uint32_t)ovf_bytes - off) return -1;
  for (uint32_t i = 0; i < len && s >= 0; ++i) s = gm_step(tr, n, s, ovf[off + i]);
  return s;
}

}  // namespace

__global__ __launch_bounds__(GM_NT) void guide_mask_kernel(
    const uint4* __restrict__ rec, const uint8_t* __restrict__ ovf, int ovf_bytes, int vocab, int words,
    const uint16_t* __restrict__ arena, const uint8_t* __restrict__ accept, int arena_states,
    const int* __restrict__ row_base, const int* __restrict__ row_nstates, const int* __restrict__ row_state,
    const int* __restrict__ pend_src, const int* __restrict__ tokens, int n_tokens,
    const uint32_t* __restrict__ base_bits, const int* __restrict__ base_idx, int n_static,
    uint32_t* __restrict__ bits, int* __restrict__ idx, int* __restrict__ state_after) {
  const int tile = blockIdx.x, row = blockIdx.y;
  const int lane = threadIdx.x & 63;
  uint32_t* out = bits + (size_t)(n_static + row) * words;
  const int b0 = row_base[row];
  int bidx = base_idx ? base_idx[row] : -1;
  const bool first = tile == 0 && threadIdx.x == 0;
  if (b0 < 0) {   // uniform: not guided
    const int w = tile * (GM_TILE / 32) + (int)threadIdx.x;
    if (threadIdx.x < GM_TILE / 32 && w < words) out[w] = 0u;
    if (first) {
      idx[row] = bidx;
      state_after[row] = -1;
    }
    return;
  }
  if (bidx >= n_static) bidx = -1;
  // the wave's first token of round j, and the word its ballot starts at
  const int wave_tok = tile * GM_TILE + ((int)threadIdx.x & ~63);
  uint4 rc[GM_UN];
  uint32_t bw[GM_UN];
#pragma unroll
  for (int j = 0; j < GM_UN; ++j) {
    const int t = wave_tok + j * GM_NT + lane;
    rc[j] = t < vocab ? rec[t] : make_uint4(0u, 0u, 0u, 0u);
    const int w = ((wave_tok + j * GM_NT) >> 5) + lane;
    bw[j] = (bidx >= 0 && lane < 2 && w < words) ? base_bits[(size_t)bidx * words + w] : 0xffffffffu;
  }
  // the states of this guide that lie inside the arena
  const int n = b0 < arena_states ? min(row_nstates[row], arena_states - b0) : 0;
  const uint16_t* tr = arena + (size_t)(n > 0 ? b0 : 0) * 256;
  int s = row_state[row];
  if (s < 0 || s >= n) s = -1;
  const int ps = pend_src ? pend_src[row] : -1;
  if (s >= 0 && ps >= 0 && ps < n_tokens) {   // the pending token: uniform over the workgroup
    const int t = tokens[ps];
    if (t < 0 || t >= vocab) {
      s = -1;
    } else {
      const uint4 pr = rec[t];
      const uint32_t code = pr.x & 31u;
      if (pr.x & GM_EOS) {
        // EOS does not move the state
      } else if (code == GM_LONG) {
        s = gm_walk_long(tr, n, s, ovf, ovf_bytes, pr.y, pr.z);
      } else if (code == 0u || code > (uint32_t)GM_INLINE) {
        s = -1;
      } else {
        for (int k = 1; k <= (int)code && s >= 0; ++k) s = gm_step(tr, n, s, rec_byte(pr, k));
      }
    }
  }
  if (first) {
    idx[row] = n_static + row;
    state_after[row] = s;
  }
  int st[GM_UN], len[GM_UN];
#pragma unroll
  for (int j = 0; j < GM_UN; ++j) {
    const uint32_t code = rc[j].x & 31u;
    len[j] = code <= (uint32_t)GM_INLINE ? (int)code : 0;
    st[j] = (s >= 0 && (len[j] > 0 || code == GM_LONG)) ? s : -1;
  }
  if (s >= 0) {   // uniform; n >= 1 here
#pragma unroll
    for (int k = 1; k <= GM_INLINE; ++k) {
      bool any = false;
#pragma unroll
      for (int j = 0; j < GM_UN; ++j) any |= k <= len[j] && st[j] >= 0;
      if (!__any(any)) break;   // no token of this wave is alive and unfinished
      int nx[GM_UN];
#pragma unroll
      for (int j = 0; j < GM_UN; ++j) nx[j] = gm_step(tr, n, st[j], rec_byte(rc[j], k));
#pragma unroll
      for (int j = 0; j < GM_UN; ++j)
        if (k <= len[j]) st[j] = nx[j];
    }
#pragma unroll
    for (int j = 0; j < GM_UN; ++j)
      if ((rc[j].x & 31u) == GM_LONG && st[j] >= 0)   // rare: a token longer than the record holds
        st[j] = gm_walk_long(tr, n, st[j], ovf, ovf_bytes, rc[j].y, rc[j].z);
  }
  const bool acc = s >= 0 && accept[b0 + s] != 0;
#pragma unroll
  for (int j = 0; j < GM_UN; ++j) {
    const int t = wave_tok + j * GM_NT + lane;
    const bool ok = t < vocab && (st[j] >= 0 || ((rc[j].x & GM_EOS) && acc));
    const unsigned long long m = __ballot(ok);
    const int w = ((wave_tok + j * GM_NT) >> 5) + lane;
    if (lane < 2 && w < words) out[w] = (lane ? (uint32_t)(m >> 32) : (uint32_t)m) & bw[j];
  }
}

// one workgroup per row: a guided row without a single bit gets eos0's
__global__ __launch_bounds__(GM_NT) void guide_mask_fixup_kernel(const int* __restrict__ row_base,
                                                                 uint32_t* __restrict__ bits, int words,
                                                                 int n_static, int eos0) {
  const int row = blockIdx.x;
  if (row_base[row] < 0) return;   // uniform
  uint32_t* out = bits + (size_t)(n_static + row) * words;
  uint32_t seen = 0u;
  for (int w = threadIdx.x; w < words; w += GM_NT) seen |= out[w];
  if (__syncthreads_or(seen != 0u)) return;
  if (threadIdx.x == 0) out[eos0 >> 5] = 1u << (eos0 & 31);
}

// tokens per workgroup: the geometry the tests straddle
extern "C" int ka_guide_mask_tile() { return GM_TILE; }

// bits uint32 [n_static + rows, ceil(vocab / 32)]: rows n_static.. are written here (the caller copies the
// SAFE_DECODE rows in front); idx, state_after int32 [rows].  rec: 16-byte records [vocab]; ovf [ovf_bytes]
// (may be null when 0).  pend_src [rows] may be null (no row has a pending token), tokens [n_tokens] then
// too; base_bits [n_static, words] with base_idx [rows], or both null.
extern "C" int ka_guide_mask(void* bits, int* idx, int* state_after, const void* rec, const void* ovf,
                             int ovf_bytes, int vocab, int eos0, const void* arena, const void* accept,
                             int arena_states, const int* row_base, const int* row_nstates, const int* row_state,
                             const int* pend_src, const int* tokens, int n_tokens, const void* base_bits,
                             const int* base_idx, int n_static, int rows, hipStream_t stream) {
  if (rows < 0 || rows > 65535 || vocab <= 0 || arena_states <= 0 || ovf_bytes < 0 || n_tokens < 0 || n_static < 0)
    return (int)hipErrorInvalidValue;
  if (eos0 < 0 || eos0 >= vocab) return (int)hipErrorInvalidValue;
  if (bits == nullptr || idx == nullptr || state_after == nullptr || rec == nullptr || arena == nullptr ||
      accept == nullptr || row_base == nullptr || row_nstates == nullptr || row_state == nullptr)
    return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(rec) & 15u) != 0 || (reinterpret_cast<uintptr_t>(bits) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(arena) & 1u) != 0)
    return (int)hipErrorInvalidValue;
  if (ovf_bytes > 0 && ovf == nullptr) return (int)hipErrorInvalidValue;
  if (pend_src != nullptr && tokens == nullptr) return (int)hipErrorInvalidValue;
  if ((base_bits == nullptr) != (base_idx == nullptr) || (base_bits == nullptr) != (n_static == 0))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  const int words = (vocab + 31) / 32;
  const int tiles = (vocab + GM_TILE - 1) / GM_TILE;
  hipLaunchKernelGGL(guide_mask_kernel, dim3(tiles, rows), dim3(GM_NT), 0, stream, static_cast<const uint4*>(rec),
                     static_cast<const uint8_t*>(ovf), ovf_bytes, vocab, words, static_cast<const uint16_t*>(arena),
                     static_cast<const uint8_t*>(accept), arena_states, row_base, row_nstates, row_state, pend_src,
                     tokens, n_tokens, static_cast<const uint32_t*>(base_bits), base_idx, n_static,
                     static_cast<uint32_t*>(bits), idx, state_after);
  hipLaunchKernelGGL(guide_mask_fixup_kernel, dim3(rows), dim3(GM_NT), 0, stream, row_base,
                     static_cast<uint32_t*>(bits), words, n_static, eos0);
  KA_CHECK_LAUNCH();
}
