// Per-request edits of a step's logits before the sampler reads them: `presence_penalty`,
// `frequency_penalty`, `repetition_penalty` and `logit_bias` of /v1/chat/completions.
//
// KA_HIPCC_FLAGS: -ffp-contract=off
// (The __f*_rn intrinsics below state that every operation is rounded on its own, but hipcc lowers them
// to plain operators, and under its default -ffp-contract=fast the backend fused frequency * c into the
// subtraction: v_fma_f32 in the device assembly, a `#pragma clang fp contract(off)` in the function did
// not stop it.  The file is compiled without contraction; the division's own expansion keeps its FMAs.)
//
// Per row the host sends a short list of entries (CSR: row_start [rows + 1]), one per token that can
// change: id (global token id, distinct within the row), cnt (bits 0-30 = c, the token's occurrences in
// the sequence's output so far; bit 31 = the token occurs in the prompt) and bias (0 without a
// logit_bias entry), and the row's presence / frequency / repetition.  With seen = c > 0 or the prompt
// bit, every operation in fp32 and rounded on its own (semantics: ops/reference.py `logit_adjust`):
//   x = float(bf16 logit)
//   if (seen && repetition != 1) x = x > 0 ? x / repetition : x * repetition
//   x = x - frequency * float(c);  x = x - (c > 0 ? presence : 0);  x = x + bias
//   logit = bf16 round-to-nearest-even(x)
// The result stays bf16: the sampler and the logprobs kernel are exact selects over the 65,536 bf16
// patterns and read these logits unchanged.  An entry outside [vocab_offset, vocab_offset + vocab) is
// skipped (ops.sample's slice convention).
//
// The pending token.  Under lookahead scheduling the newest output token of a row may exist only on
// the device: pend_src[row] >= 0 says it is tokens[pend_src[row]] and the entries do not count it.  It
// gets c + 1 and seen; the thread that owns an entry with that id applies it there, otherwise one
// thread handles it after a workgroup barrier as one more entry (c = 1, no prompt bit, bias 0): once
// either way.  A row with no entries is left alone when it has no pending token or its three
// parameters are neutral (the pending token would change nothing).
//
// One workgroup per row.  A thread takes LA_UN entries per round: the id / cnt / bias loads of the
// whole batch are issued first, then the batch's 2-byte logit gathers, then the arithmetic and the
// 2-byte stores (a rolled loop would wait three times per entry: docs/ARCHITECTURE.md, latency-bound
// kernels).  A logit is written with a 16-bit store, never by a read-modify-write of its dword: the
// neighbouring token may be another thread's.
//
// saved (ka_logit_adjust: optional; ka_logit_restore: required), bf16 [rows + entries]: slot `row` holds
// the original pattern of the row's pending token when no entry has its id, slot rows + e that of
// entry e.  ka_logit_restore follows the same rules and writes those patterns back: a step that also
// reports log-probabilities runs it between the sampler and ka_token_logprobs, which describe the
// unadjusted distribution.
#include "common.h"

namespace {

constexpr int LA_NT = 256;
constexpr int LA_UN = 8;
constexpr uint32_t LA_PROMPT_BIT = 0x80000000u;

KA_DEV bf16_t adjust_one(bf16_t raw, int c, bool prompt, float bias, float presence, float frequency,
                         float repetition) {
  // every operation rounds on its own: see the note on KA_HIPCC_FLAGS in the header
  float x = bf2f(raw);
  if ((prompt || c > 0) && repetition != 1.f) x = x > 0.f ? __fdiv_rn(x, repetition) : __fmul_rn(x, repetition);
  x = __fsub_rn(x, __fmul_rn(frequency, (float)c));
  x = __fsub_rn(x, c > 0 ? presence : 0.f);
  x = __fadd_rn(x, bias);
  return f2bf(x);
}

}  // namespace

template <bool RESTORE>
__global__ __launch_bounds__(LA_NT) void logit_adjust_kernel(
    bf16_t* __restrict__ logits, const int* __restrict__ row_start, const int* __restrict__ ent_id,
    const int* __restrict__ ent_cnt, const float* __restrict__ ent_bias, const float* __restrict__ presence,
    const float* __restrict__ frequency, const float* __restrict__ repetition, const int* __restrict__ pend_src,
    const int* __restrict__ tokens, int n_tokens, bf16_t* __restrict__ saved, int rows, int entries, int vocab,
    int vocab_offset) {
  __shared__ int s_found;
  const int row = blockIdx.x;
  const int e0 = max(0, row_start[row]), e1 = min(entries, row_start[row + 1]);
  const int ps = pend_src ? pend_src[row] : -1;
  const float pres = presence[row], freq = frequency[row], rep = repetition[row];
  const bool has_pend = ps >= 0 && ps < n_tokens;
  if (e0 >= e1 && (!has_pend || (pres == 0.f && freq == 0.f && rep == 1.f))) return;   // uniform over the workgroup
  // the pending token's index in this slice, -1: none, or outside the slice
  int pend = -1;
  if (has_pend) {
    const int li = tokens[ps] - vocab_offset;
    pend = (li >= 0 && li < vocab) ? li : -1;
  }
  if (threadIdx.x == 0) s_found = 0;
  __syncthreads();
  bf16_t* lr = logits + (size_t)row * vocab;
  bf16_t* sv = saved ? saved + rows : nullptr;
  bool found = false;
  for (int base = e0 + threadIdx.x; base < e1; base += LA_NT * LA_UN) {
    int li[LA_UN], cnt[LA_UN];
    float bias[LA_UN];
    bf16_t raw[LA_UN];
#pragma unroll
    for (int j = 0; j < LA_UN; ++j) {
      const int e = base + j * LA_NT;
      li[j] = -1;
      cnt[j] = 0;
      bias[j] = 0.f;
      if (e < e1) {
        li[j] = ent_id[e] - vocab_offset;
        if (!RESTORE) {
          cnt[j] = ent_cnt[e];
          bias[j] = ent_bias[e];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < LA_UN; ++j) {
      if (li[j] < 0 || li[j] >= vocab) li[j] = -1;   // past the segment, or an id outside the slice
      raw[j] = 0;
      if (li[j] >= 0) raw[j] = RESTORE ? sv[base + j * LA_NT] : lr[li[j]];
    }
#pragma unroll
    for (int j = 0; j < LA_UN; ++j) {
      if (li[j] < 0) continue;
      const bool is_pend = li[j] == pend;
      found |= is_pend;
      if (RESTORE) {
        lr[li[j]] = raw[j];
      } else {
        const int c = (int)((uint32_t)cnt[j] & ~LA_PROMPT_BIT) + (is_pend ? 1 : 0);
        if (sv) sv[base + j * LA_NT] = raw[j];
        lr[li[j]] = adjust_one(raw[j], c, ((uint32_t)cnt[j] & LA_PROMPT_BIT) != 0u, bias[j], pres, freq, rep);
      }
    }
  }
  if (pend < 0) return;   // uniform: the barrier below is the pending token's alone
  if (found) s_found = 1;   // ids are distinct within a row: at most one thread
  __syncthreads();
  if (threadIdx.x == 0 && !s_found) {
    if (RESTORE) {
      lr[pend] = saved[row];
    } else {
      const bf16_t raw = lr[pend];
      if (saved) saved[row] = raw;
      lr[pend] = adjust_one(raw, 1, false, 0.f, pres, freq, rep);
    }
  }
}

namespace {

template <bool RESTORE>
int launch(void* logits, const int* row_start, const int* ent_id, const int* ent_cnt, const float* ent_bias,
           const float* presence, const float* frequency, const float* repetition, const int* pend_src,
           const int* tokens, int n_tokens, void* saved, int rows, int entries, int vocab, int vocab_offset,
           hipStream_t stream) {
  if (rows < 0 || entries < 0 || vocab <= 0 || n_tokens < 0) return (int)hipErrorInvalidValue;
  if (logits == nullptr || row_start == nullptr || presence == nullptr || frequency == nullptr ||
      repetition == nullptr || (RESTORE && saved == nullptr))
    return (int)hipErrorInvalidValue;
  if (entries > 0 && (ent_id == nullptr || (!RESTORE && (ent_cnt == nullptr || ent_bias == nullptr))))
    return (int)hipErrorInvalidValue;
  if (pend_src != nullptr && tokens == nullptr) return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(logit_adjust_kernel<RESTORE>, dim3(rows), dim3(LA_NT), 0, stream, static_cast<bf16_t*>(logits),
                     row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src, tokens, n_tokens,
                     static_cast<bf16_t*>(saved), rows, entries, vocab, vocab_offset);
  KA_CHECK_LAUNCH();
}

}  // namespace

// entries per thread and round times the workgroup size: the geometry the tests straddle
extern "C" int ka_logit_adjust_batch() { return LA_NT * LA_UN; }
extern "C" int ka_logit_adjust_threads() { return LA_NT; }

// logits bf16 [rows, vocab], edited in place.  ent_* [entries] (may be null when entries == 0); pend_src
// [rows] may be null (no row has a pending token), tokens [n_tokens] then too; saved bf16 [rows + entries]
// or null.
extern "C" int ka_logit_adjust(void* logits, const int* row_start, const int* ent_id, const int* ent_cnt,
                               const float* ent_bias, const float* presence, const float* frequency,
                               const float* repetition, const int* pend_src, const int* tokens, int n_tokens,
                               void* saved, int rows, int entries, int vocab, int vocab_offset, hipStream_t stream) {
  return launch<false>(logits, row_start, ent_id, ent_cnt, ent_bias, presence, frequency, repetition, pend_src, tokens,
                       n_tokens, saved, rows, entries, vocab, vocab_offset, stream);
}

// writes back what ka_logit_adjust saved, from the same image and the same `tokens`
extern "C" int ka_logit_restore(void* logits, const int* row_start, const int* ent_id, const float* presence,
                                const float* frequency, const float* repetition, const int* pend_src,
                                const int* tokens, int n_tokens, const void* saved, int rows, int entries, int vocab,
                                int vocab_offset, hipStream_t stream) {
  return launch<true>(logits, row_start, ent_id, nullptr, nullptr, presence, frequency, repetition, pend_src, tokens,
                      n_tokens, const_cast<void*>(saved), rows, entries, vocab, vocab_offset, stream);
}
