// Guided decoding with a stack (JSON mode: `response_format`, `guided_json`): guide_mask.hip's per-row vocabulary
// bitmask for a step that holds rows under a stack guide (engine/guided.py StackGuide).  A byte-level DFA cannot
// count brackets, so here every row carries a stack of up to 64 four-bit symbols and every token walks with a
// stack of its own on top of it.  Semantics: ops/reference.py `guide_mask_stack`.  Everything is integer.
//
// Token table, DFA arena, grid (vocabulary tile, row), GS_NT threads, GS_UN rounds of one token per lane, the
// 128-bit record loads, the ballot stores and the fallback kernel are guide_mask.hip's.  Added per row: row_kind
// (0: a DFA row, guide_mask's entry semantics exactly; 1: a stack row), row_depth, row_stack (8 words: 64 symbols,
// bottom first, symbol i in bits 4 (i mod 8) of word i / 8), and arena_pop uint16 [arena_states, 16], whose row
// `base` is the guide's pop_to.  An entry e of a stack row: bit 15 = pop (push bits must be 0, the stack not
// empty; the next state is pop_to[top symbol]); else bits 0-10 = the next state and bits 11-14 = a symbol 1..14
// to push (0 = none, 15 = dead).  A push at depth 64, and a 17th live push of one token, are dead.
//
// The workgroup unpacks the row's stack into LDS, one symbol per byte, and checks it (a depth outside 0..64, a
// symbol 0 or 15 below the depth: the row is dead).  Thread 0 walks the pending token on that LDS stack and
// publishes state and depth; thread 0 of tile 0 writes state_after / depth_after / stack_after.  Then the tokens:
// per token, in registers, the state, a 64-bit shift register of the symbols the token itself has pushed (newest
// in the low four bits), their count, and the number of symbols it has consumed from the row's stack.  A pop
// takes from the register while it holds any, else the byte at depth - 1 - consumed of the LDS stack (a per-lane
// LDS read, never a write: the row's stack is shared and read-only during the token walk).  Per byte position the
// GS_UN table lookups are issued first and the stack updates applied after, so the dependent-load latency is still
// hidden by GS_UN independent loads per lane (docs/ARCHITECTURE.md, latency-bound kernels).
// Every lookup is guarded: a state only inside [0, n), a token id inside [0, vocab), an overflow run inside the
// pool, a row-stack index inside [0, 64), a pop_to index inside 1..14.
#include "common.h"

namespace {

constexpr int GS_NT = 256;
constexpr int GS_UN = 4;
constexpr int GS_TILE = GS_NT * GS_UN;   // tokens per workgroup
constexpr uint32_t GS_EOS = 0x80u;
constexpr uint32_t GS_LONG = 31u;
constexpr int GS_INLINE = 15;
constexpr int GS_DEPTH = 64;             // symbols on a row's stack
constexpr int GS_OWN = 16;               // live pushes of one token
constexpr uint32_t GS_POP = 0x8000u;

KA_DEV uint32_t gs_rec_byte(const uint4& r, int k) {
  const uint32_t w = k < 4 ? r.x : k < 8 ? r.y : k < 12 ? r.z : r.w;
  return (w >> (8 * (k & 3))) & 0xffu;
}

// one token's walk
struct GsTok {
  int s;                     // state, -1 = dead
  unsigned long long reg;    // the symbols this token pushed, newest in bits 0-3
  int cnt;                   // how many of them
  int cons;                  // symbols taken from the row's stack
};

// the entry under byte b; a dead lane reads state 0's row (n >= 1: callers check) and discards it
KA_DEV uint32_t gs_load(const uint16_t* __restrict__ tr, int n, int s, uint32_t b) {
  return tr[(size_t)((s >= 0 && s < n) ? s : 0) * 256 + b];
}

// apply entry e to t.  sym: the row's stack in LDS (depth symbols), pop: the guide's pop_to in LDS
KA_DEV void gs_apply(GsTok& t, uint32_t e, int n, bool stacked, int depth, const uint8_t* sym, const uint16_t* pop) {
  const bool live = t.s >= 0 && t.s < n;
  int nx = -1;
  if (!stacked) {
    if (live && e < (uint32_t)n) nx = (int)e;
  } else if (live) {
    const uint32_t y = (e >> 11) & 15u;
    const int d = depth - t.cons + t.cnt;
    if (e & GS_POP) {
      if (y == 0u && d > 0) {
        uint32_t top = 0u;
        if (t.cnt > 0) {
          top = (uint32_t)(t.reg & 15ull);
          t.reg >>= 4;
          --t.cnt;
        } else {
          const int at = depth - 1 - t.cons;
          if (at >= 0 && at < GS_DEPTH) top = sym[at];
          ++t.cons;
        }
        if (top >= 1u && top <= 14u) {
          const uint32_t to = pop[top];
          if (to < (uint32_t)n) nx = (int)to;
        }
      }
    } else {
      const uint32_t tgt = e & 0x7ffu;
      if (tgt < (uint32_t)n && y != 15u) {
        if (y == 0u) {
          nx = (int)tgt;
        } else if (d < GS_DEPTH && t.cnt < GS_OWN) {
          t.reg = (t.reg << 4) | y;
          ++t.cnt;
          nx = (int)tgt;
        }
      }
    }
  }
  t.s = nx;
}

KA_DEV void gs_walk_long(GsTok& t, const uint16_t* __restrict__ tr, int n, bool stacked, int depth,
                         const uint8_t* sym, const uint16_t* pop, const uint8_t* __restrict__ ovf, int ovf_bytes,
                         uint32_t off, uint32_t len) {
  if (len == 0u || off > (uint32_t)ovf_bytes || len > (uint32_t)ovf_bytes - off) {
    t.s = -1;
    return;
  }
  for (uint32_t i = 0; i < len && t.s >= 0; ++i) gs_apply(t, gs_load(tr, n, t.s, ovf[off + i]), n, stacked, depth, sym, pop);
}

// thread 0: one byte of the pending token, on the LDS stack itself (d symbols, own of them pushed by this token)
KA_DEV int gs_pend_step(const uint16_t* __restrict__ tr, int n, bool stacked, int s, uint32_t b, uint8_t* sym,
                        const uint16_t* pop, int& d, int& own) {
  if (s < 0 || s >= n) return -1;
  const uint32_t e = tr[(size_t)s * 256 + b];
  if (!stacked) return e < (uint32_t)n ? (int)e : -1;
  const uint32_t y = (e >> 11) & 15u;
  if (e & GS_POP) {
    if (y != 0u || d <= 0 || d > GS_DEPTH) return -1;
    const uint32_t top = sym[--d];
    if (own > 0) --own;
    if (top < 1u || top > 14u) return -1;
    const uint32_t to = pop[top];
    return to < (uint32_t)n ? (int)to : -1;
  }
  const uint32_t tgt = e & 0x7ffu;
  if (tgt >= (uint32_t)n || y == 15u) return -1;
  if (y != 0u) {
    if (d < 0 || d >= GS_DEPTH || own >= GS_OWN) return -1;
    sym[d++] = (uint8_t)y;
    ++own;
  }
  return (int)tgt;
}

}  // namespace

__global__ __launch_bounds__(GS_NT) void guide_stack_kernel(
    const uint4* __restrict__ rec, const uint8_t* __restrict__ ovf, int ovf_bytes, int vocab, int words,
    const uint16_t* __restrict__ arena, const uint8_t* __restrict__ accept, const uint16_t* __restrict__ arena_pop,
    int arena_states, const int* __restrict__ row_base, const int* __restrict__ row_nstates,
    const int* __restrict__ row_state, const int* __restrict__ row_kind, const int* __restrict__ row_depth,
    const uint32_t* __restrict__ row_stack, const int* __restrict__ pend_src, const int* __restrict__ tokens,
    int n_tokens, const uint32_t* __restrict__ base_bits, const int* __restrict__ base_idx, int n_static,
    uint32_t* __restrict__ bits, int* __restrict__ idx, int* __restrict__ state_after, int* __restrict__ depth_after,
    uint32_t* __restrict__ stack_after) {
  __shared__ uint8_t s_sym[GS_DEPTH];
  __shared__ uint16_t s_pop[16];
  __shared__ int s_pub[2];   // state and depth after the pending token
  const int tile = blockIdx.x, row = blockIdx.y;
  const int lane = threadIdx.x & 63;
  uint32_t* out = bits + (size_t)(n_static + row) * words;
  const int b0 = row_base[row];
  int bidx = base_idx ? base_idx[row] : -1;
  const bool first = tile == 0 && threadIdx.x == 0;
  if (b0 < 0) {   // uniform: not guided
    const int w = tile * (GS_TILE / 32) + (int)threadIdx.x;
    if (threadIdx.x < GS_TILE / 32 && w < words) out[w] = 0u;
    if (first) {
      idx[row] = bidx;
      state_after[row] = -1;
      depth_after[row] = 0;
    }
    if (tile == 0 && threadIdx.x < 8) stack_after[(size_t)row * 8 + threadIdx.x] = 0u;
    return;
  }
  if (bidx >= n_static) bidx = -1;
  const int wave_tok = tile * GS_TILE + ((int)threadIdx.x & ~63);
  uint4 rc[GS_UN];
  uint32_t bw[GS_UN];
#pragma unroll
  for (int j = 0; j < GS_UN; ++j) {
    const int t = wave_tok + j * GS_NT + lane;
    rc[j] = t < vocab ? rec[t] : make_uint4(0u, 0u, 0u, 0u);
    const int w = ((wave_tok + j * GS_NT) >> 5) + lane;
    bw[j] = (bidx >= 0 && lane < 2 && w < words) ? base_bits[(size_t)bidx * words + w] : 0xffffffffu;
  }
  const int n = b0 < arena_states ? min(row_nstates[row], arena_states - b0) : 0;
  const uint16_t* tr = arena + (size_t)(n > 0 ? b0 : 0) * 256;
  const bool stacked = row_kind[row] == 1;   // uniform
  const int d0 = stacked ? row_depth[row] : 0;
  // the row's stack, one symbol per byte, and the guide's pop_to
  bool bad = false;
  if (threadIdx.x < GS_DEPTH) {
    uint32_t y = 0u;
    if (stacked) y = (row_stack[(size_t)row * 8 + (threadIdx.x >> 3)] >> (4 * (threadIdx.x & 7))) & 15u;
    s_sym[threadIdx.x] = (uint8_t)y;
    bad = stacked && (int)threadIdx.x < d0 && (y == 0u || y == 15u);
  } else if (threadIdx.x < GS_DEPTH + 16) {
    const int i = (int)threadIdx.x - GS_DEPTH;
    s_pop[i] = (stacked && n > 0) ? arena_pop[(size_t)b0 * 16 + i] : (uint16_t)0xffffu;
  }
  bad = __syncthreads_or(bad) != 0 || d0 < 0 || d0 > GS_DEPTH;
  if (threadIdx.x == 0) {
    int s = row_state[row];
    int d = d0, own = 0;
    if (s < 0 || s >= n || bad) s = -1;
    const int ps = pend_src ? pend_src[row] : -1;
    if (s >= 0 && ps >= 0 && ps < n_tokens) {   // the pending token
      const int t = tokens[ps];
      if (t < 0 || t >= vocab) {
        s = -1;
      } else {
        const uint4 pr = rec[t];
        const uint32_t code = pr.x & 31u;
        if (pr.x & GS_EOS) {
          // EOS moves neither the state nor the stack
        } else if (code == GS_LONG) {
          const uint32_t off = pr.y, len = pr.z;
          if (len == 0u || off > (uint32_t)ovf_bytes || len > (uint32_t)ovf_bytes - off) {
            s = -1;
          } else {
            for (uint32_t i = 0; i < len && s >= 0; ++i) s = gs_pend_step(tr, n, stacked, s, ovf[off + i], s_sym, s_pop, d, own);
          }
        } else if (code == 0u || code > (uint32_t)GS_INLINE) {
          s = -1;
        } else {
          for (int k = 1; k <= (int)code && s >= 0; ++k) s = gs_pend_step(tr, n, stacked, s, gs_rec_byte(pr, k), s_sym, s_pop, d, own);
        }
      }
    }
    if (s < 0 || !stacked) d = 0;
    s_pub[0] = s;
    s_pub[1] = d;
    if (tile == 0) {
      idx[row] = n_static + row;
      state_after[row] = s;
      depth_after[row] = d;
      for (int w = 0; w < 8; ++w) {
        uint32_t v = 0u;
        for (int i = 0; i < 8; ++i)
          if (w * 8 + i < d) v |= (uint32_t)s_sym[w * 8 + i] << (4 * i);
        stack_after[(size_t)row * 8 + w] = v;
      }
    }
  }
  __syncthreads();
  const int s = s_pub[0];
  const int depth = s_pub[1];
  GsTok tk[GS_UN];
  int len[GS_UN];
#pragma unroll
  for (int j = 0; j < GS_UN; ++j) {
    const uint32_t code = rc[j].x & 31u;
    len[j] = code <= (uint32_t)GS_INLINE ? (int)code : 0;
    tk[j].s = (s >= 0 && (len[j] > 0 || code == GS_LONG)) ? s : -1;
    tk[j].reg = 0ull;
    tk[j].cnt = 0;
    tk[j].cons = 0;
  }
  if (s >= 0) {   // uniform; n >= 1 here
#pragma unroll
    for (int k = 1; k <= GS_INLINE; ++k) {
      bool any = false;
#pragma unroll
      for (int j = 0; j < GS_UN; ++j) any |= k <= len[j] && tk[j].s >= 0;
      if (!__any(any)) break;   // no token of this wave is alive and unfinished
      uint32_t e[GS_UN];
#pragma unroll
      for (int j = 0; j < GS_UN; ++j) e[j] = gs_load(tr, n, tk[j].s, gs_rec_byte(rc[j], k));
#pragma unroll
      for (int j = 0; j < GS_UN; ++j)
        if (k <= len[j]) gs_apply(tk[j], e[j], n, stacked, depth, s_sym, s_pop);
    }
#pragma unroll
    for (int j = 0; j < GS_UN; ++j)
      if ((rc[j].x & 31u) == GS_LONG && tk[j].s >= 0)   // rare: a token longer than the record holds
        gs_walk_long(tk[j], tr, n, stacked, depth, s_sym, s_pop, ovf, ovf_bytes, rc[j].y, rc[j].z);
  }
  const bool acc = s >= 0 && accept[b0 + s] != 0;
#pragma unroll
  for (int j = 0; j < GS_UN; ++j) {
    const int t = wave_tok + j * GS_NT + lane;
    const bool ok = t < vocab && (tk[j].s >= 0 || ((rc[j].x & GS_EOS) && acc));
    const unsigned long long m = __ballot(ok);
    const int w = ((wave_tok + j * GS_NT) >> 5) + lane;
    if (lane < 2 && w < words) out[w] = (lane ? (uint32_t)(m >> 32) : (uint32_t)m) & bw[j];
  }
}

// one workgroup per row: a guided row without a single bit gets eos0's
__global__ __launch_bounds__(GS_NT) void guide_stack_fixup_kernel(const int* __restrict__ row_base,
                                                                  uint32_t* __restrict__ bits, int words,
                                                                  int n_static, int eos0) {
  const int row = blockIdx.x;
  if (row_base[row] < 0) return;   // uniform
  uint32_t* out = bits + (size_t)(n_static + row) * words;
  uint32_t seen = 0u;
  for (int w = threadIdx.x; w < words; w += GS_NT) seen |= out[w];
  if (__syncthreads_or(seen != 0u)) return;
  if (threadIdx.x == 0) out[eos0 >> 5] = 1u << (eos0 & 31);
}

// tokens per workgroup: the geometry the tests straddle
extern "C" int ka_guide_mask_stack_tile() { return GS_TILE; }

// ka_guide_mask's arguments, plus arena_pop uint16 [arena_states, 16], row_kind / row_depth int32 [rows],
// row_stack uint32 [rows, 8] and the outputs depth_after int32 [rows], stack_after uint32 [rows, 8].
extern "C" int ka_guide_mask_stack(void* bits, int* idx, int* state_after, int* depth_after, void* stack_after,
                                   const void* rec, const void* ovf, int ovf_bytes, int vocab, int eos0,
                                   const void* arena, const void* accept, const void* arena_pop, int arena_states,
                                   const int* row_base, const int* row_nstates, const int* row_state,
                                   const int* row_kind, const int* row_depth, const void* row_stack,
                                   const int* pend_src, const int* tokens, int n_tokens, const void* base_bits,
                                   const int* base_idx, int n_static, int rows, hipStream_t stream) {
  if (rows < 0 || rows > 65535 || vocab <= 0 || arena_states <= 0 || ovf_bytes < 0 || n_tokens < 0 || n_static < 0)
    return (int)hipErrorInvalidValue;
  if (eos0 < 0 || eos0 >= vocab) return (int)hipErrorInvalidValue;
  if (bits == nullptr || idx == nullptr || state_after == nullptr || depth_after == nullptr ||
      stack_after == nullptr || rec == nullptr || arena == nullptr || accept == nullptr || arena_pop == nullptr ||
      row_base == nullptr || row_nstates == nullptr || row_state == nullptr || row_kind == nullptr ||
      row_depth == nullptr || row_stack == nullptr)
    return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(rec) & 15u) != 0 || (reinterpret_cast<uintptr_t>(bits) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(arena) & 1u) != 0 || (reinterpret_cast<uintptr_t>(arena_pop) & 1u) != 0 ||
      (reinterpret_cast<uintptr_t>(row_stack) & 3u) != 0 || (reinterpret_cast<uintptr_t>(stack_after) & 3u) != 0)
    return (int)hipErrorInvalidValue;
  if (ovf_bytes > 0 && ovf == nullptr) return (int)hipErrorInvalidValue;
  if (pend_src != nullptr && tokens == nullptr) return (int)hipErrorInvalidValue;
  if ((base_bits == nullptr) != (base_idx == nullptr) || (base_bits == nullptr) != (n_static == 0))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  const int words = (vocab + 31) / 32;
  const int tiles = (vocab + GS_TILE - 1) / GS_TILE;
  hipLaunchKernelGGL(guide_stack_kernel, dim3(tiles, rows), dim3(GS_NT), 0, stream, static_cast<const uint4*>(rec),
                     static_cast<const uint8_t*>(ovf), ovf_bytes, vocab, words, static_cast<const uint16_t*>(arena),
                     static_cast<const uint8_t*>(accept), static_cast<const uint16_t*>(arena_pop), arena_states,
                     row_base, row_nstates, row_state, row_kind, row_depth, static_cast<const uint32_t*>(row_stack),
                     pend_src, tokens, n_tokens, static_cast<const uint32_t*>(base_bits), base_idx, n_static,
                     static_cast<uint32_t*>(bits), idx, state_after, depth_after, static_cast<uint32_t*>(stack_after));
  hipLaunchKernelGGL(guide_stack_fixup_kernel, dim3(rows), dim3(GS_NT), 0, stream, row_base,
                     static_cast<uint32_t*>(bits), words, n_static, eos0);
  KA_CHECK_LAUNCH();
}
