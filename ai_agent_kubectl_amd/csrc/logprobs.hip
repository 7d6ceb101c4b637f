// Per-token log-probabilities (and the top-n alternatives) of a step's logits under the SAFE_DECODE
// token mask: what /v1/chat/completions reports as `logprobs` / `top_logprobs`.
//
// Per row (A = tokens the mask allows, l_i = the bf16 logit as fp32):
//   m = max over A of l_i;  w_i = expf(l_i - m);  mass = sum over A of trunc(w_i * 2^40) as u64;
//   S = mass * 2^-40;  logprob(i) = (l_i - m) - logf(S) for i in A, -inf outside A or outside the slice.
// This is the model's distribution under the mask BEFORE temperature / top-k / top-p (they shape the
// draw in sampling_stochastic.hip, not what is reported here).  A weight below 2^-40 counts as zero,
// so a row dominated by one token has mass == 2^40 and that token's logprob is exactly 0.
//   top_n (0..20): the n tokens of A with the largest l_i, ordered by (l_i descending, global id
//   ascending), each with its logprob; trailing entries (id -1, -inf) when A holds fewer.
//
// Every output of a row has the same bits whatever the row count, the slice count or the other rows:
// the maximum is taken in a pass of its own (every slice then uses the same m), the mass is an integer
// sum, and the top-n is a selection on exact keys.  Three launches over a grid of rows x slices
// (ka_argmax_slices, as the argmax and the sampler are sliced):
//   1. logprob_max_kernel: per slice, the largest key and the number of allowed tokens;
//   2. logprob_slice_kernel: per slice, the mass, and (top_n > 0) the slice's own first min(n, allowed)
//      tokens in that order.  The cut is the sampler's two-level radix select on the 16-bit key (256
//      LDS bins on the high byte, 256 on the low byte inside the chosen bin); the third pass takes every
//      token above the cut (fewer than n) and, of the tokens AT the cut, the lowest ids: those are
//      ranked by an ordered prefix count over the slice (512 vectors per round, lane order = id order),
//      so a row of equal logits costs no more than any other and the LDS list never exceeds n entries;
//   3. logprob_finish_kernel: one wave per row; lane s walks slice s's sorted list and the wave merges
//      them n times by a 64-lane minimum; it also sums the masses and counts and reads the chosen token
//      (`token`, the sampler's output, on the device).
// out_max / out_mass (with vocab_offset) are what a vocab-parallel combine across TP ranks would need.
#include "sampling_common.h"

namespace {

constexpr int LP_MAX_TOP = 20;
constexpr float TWO40 = 1099511627776.f;
constexpr float INV_TWO40 = 9.094947017729282379150390625e-13f;
constexpr unsigned long long SK_NONE = ~0ull;

// ascending order of the sort key = (logit descending, id ascending)
KA_DEV unsigned long long sort_key(uint32_t key, int id) {
  return ((unsigned long long)(0xffffu - key) << 32) | (unsigned long long)(uint32_t)id;
}

KA_DEV unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

struct RowSlice {
  const bf16_t* lr;
  const uint32_t* mrow;
  int v0, nvec;
};

KA_DEV RowSlice row_slice(const bf16_t* logits, const uint32_t* mask_bits, const int* mask_idx, int vocab,
                          int mask_words) {
  const int row = blockIdx.x;
  const int mi = mask_idx ? mask_idx[row] : -1;
  const int nvec_all = vocab >> 3;
  const int per = (nvec_all + gridDim.y - 1) / gridDim.y;
  const int v0 = blockIdx.y * per;
  return {logits + (size_t)row * vocab, mi >= 0 ? mask_bits + (size_t)mi * mask_words : nullptr, v0,
          min(nvec_all, v0 + per)};
}

}  // namespace

__global__ __launch_bounds__(SAMPLE_NT) void logprob_max_kernel(
    uint32_t* __restrict__ part_key, int* __restrict__ part_cnt, const bf16_t* __restrict__ logits,
    const uint32_t* __restrict__ mask_bits, const int* __restrict__ mask_idx, int vocab, int mask_words,
    int vocab_offset) {
  __shared__ uint32_t sk[SAMPLE_WAVES];
  __shared__ int sc[SAMPLE_WAVES];
  const RowSlice rs = row_slice(logits, mask_bits, mask_idx, vocab, mask_words);
  uint32_t mk = 0u;
  int cnt = 0;
  scan_row(rs.lr, rs.mrow, rs.v0, rs.nvec, vocab_offset, [&](int, uint32_t b, float) {
    mk = max(mk, bf16_key(b));
    ++cnt;
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mk = max(mk, (uint32_t)__shfl_xor((int)mk, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sk[threadIdx.x >> 6] = mk;
    sc[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < SAMPLE_WAVES; ++i) {
      mk = max(mk, sk[i]);
      cnt += sc[i];
    }
    const int p = blockIdx.x * gridDim.y + blockIdx.y;
    part_key[p] = mk;
    part_cnt[p] = cnt;
  }
}

__global__ __launch_bounds__(SAMPLE_NT) void logprob_slice_kernel(
    unsigned long long* __restrict__ part_mass, unsigned long long* __restrict__ cand, int* __restrict__ cand_cnt,
    const uint32_t* __restrict__ part_key, const int* __restrict__ part_cnt, const bf16_t* __restrict__ logits,
    const uint32_t* __restrict__ mask_bits, const int* __restrict__ mask_idx, int vocab, int mask_words,
    int vocab_offset, int top_n) {
  __shared__ Hist hist;
  __shared__ unsigned long long s_red[SAMPLE_WAVES];
  __shared__ unsigned long long s_list[LP_MAX_TOP];
  __shared__ int s_wcnt[SAMPLE_WAVES];
  __shared__ int s_sel[4];
  __shared__ int s_n;

  const RowSlice rs = row_slice(logits, mask_bits, mask_idx, vocab, mask_words);
  const int slices = gridDim.y;
  const int p = blockIdx.x * slices + blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_here = part_cnt[p];
  if (n_here == 0) {   // nothing allowed in this slice (uniform over the workgroup)
    if (threadIdx.x == 0) {
      part_mass[p] = 0ull;
      cand_cnt[p] = 0;
    }
    return;
  }
  // the row's maximum: the same m in every slice
  uint32_t mk = 0u;
  for (int i = 0; i < slices; ++i) mk = max(mk, part_key[blockIdx.x * slices + i]);
  const float m = key_value(mk);

  // ---- pass 1: the mass, and counts per high byte ----
  if (top_n > 0) hist_clear(hist);
  unsigned long long acc = 0ull;
  scan_row(rs.lr, rs.mrow, rs.v0, rs.nvec, vocab_offset, [&](int, uint32_t b, float x) {
    acc += (unsigned long long)(expf(x - m) * TWO40);
    if (top_n > 0) atomicAdd(&hist.cnt[wave][bf16_key(b) >> 8], 1u);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += shfl_xor_u64(acc, o);
  if (lane == 0) s_red[wave] = acc;
  if (top_n == 0) {
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 1; i < SAMPLE_WAVES; ++i) acc += s_red[i];
      part_mass[p] = acc;
      cand_cnt[p] = 0;
    }
    return;
  }
  hist_fold(hist);
  if (threadIdx.x == 0) {
    for (int i = 1; i < SAMPLE_WAVES; ++i) acc += s_red[i];
    part_mass[p] = acc;
    const int k = min(top_n, n_here);
    int above = 0, bin = 0;
    for (int i = 255; i >= 0; --i) {
      const int c = (int)hist.cnt[0][i];
      if (c > 0 && above + c >= k) {
        bin = i;
        break;
      }
      above += c;
    }
    s_sel[0] = bin;
    s_sel[1] = above;
    s_sel[2] = k;
  }
  __syncthreads();
  // ---- pass 2: counts per low byte inside the chosen bin -> the cut ----
  const uint32_t hb = (uint32_t)s_sel[0];
  const int above_k = s_sel[1], k = s_sel[2];
  hist_clear(hist);
  scan_row(rs.lr, rs.mrow, rs.v0, rs.nvec, vocab_offset, [&](int, uint32_t b, float) {
    const uint32_t ky = bf16_key(b);
    if ((ky >> 8) == hb) atomicAdd(&hist.cnt[wave][ky & 0xffu], 1u);
  });
  hist_fold(hist);
  if (threadIdx.x == 0) {
    int gt = above_k, lo = 0;   // gt: tokens strictly above the cut (< k)
    for (int i = 255; i >= 0; --i) {
      const int c = (int)hist.cnt[0][i];
      if (c > 0 && gt + c >= k) {
        lo = i;
        break;
      }
      gt += c;
    }
    s_sel[0] = (int)((hb << 8) | (uint32_t)lo);
    s_sel[1] = k - gt;   // tokens to take at the cut: the lowest ids
    s_n = 0;
  }
  __syncthreads();
  const uint32_t cut = (uint32_t)s_sel[0];
  int ties_left = s_sel[1];   // uniform over the workgroup
  // ---- pass 3: everything above the cut, and the first ties_left tokens at it in id order ----
  for (int base = rs.v0; base < rs.nvec; base += SAMPLE_NT) {
    const int v = base + threadIdx.x;
    uint32_t bits = 0u, eq = 0u;
    if (v < rs.nvec) {
      const int gb = (v << 3) + vocab_offset;
      bits = rs.mrow ? (rs.mrow[gb >> 5] >> (gb & 31)) & 0xffu : 0xffu;
    }
    if (bits) {
      const uint4 q = *reinterpret_cast<const uint4*>(rs.lr + ((size_t)v << 3));
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!((bits >> j) & 1u)) continue;
        const uint32_t ky = bf16_key((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu));
        if (ky > cut) {
          const int pos = atomicAdd(&s_n, 1);
          if (pos < LP_MAX_TOP) s_list[pos] = sort_key(ky, (v << 3) + j);
        } else if (ky == cut) {
          eq |= 1u << j;
        }
      }
    }
    if (ties_left > 0) {
      const int c = __popc(eq);
      if (__syncthreads_or(c)) {
        int incl = c;   // inclusive prefix over the wave: lane order is id order within a round
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(incl, o, 64);
          if (lane >= o) incl += t;
        }
        if (lane == 63) s_wcnt[wave] = incl;
        __syncthreads();
        int rank = incl - c, total = 0;
        for (int i = 0; i < SAMPLE_WAVES; ++i) {
          if (i < wave) rank += s_wcnt[i];
          total += s_wcnt[i];
        }
        for (uint32_t e = eq; e != 0u && rank < ties_left; e &= e - 1u, ++rank) {
          const int pos = atomicAdd(&s_n, 1);
          if (pos < LP_MAX_TOP) s_list[pos] = sort_key(cut, (v << 3) + (__ffs(e) - 1));
        }
        ties_left -= min(ties_left, total);
        __syncthreads();   // s_wcnt is rewritten in the next round
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = min(s_n, LP_MAX_TOP);   // == k
    unsigned long long* out = cand + (size_t)p * top_n;
    for (int i = 0; i < n; ++i) {   // insertion sort of at most 20 keys, straight into the slice's list
      const unsigned long long x = s_list[i];
      int j = i;
      for (; j > 0 && out[j - 1] > x; --j) out[j] = out[j - 1];
      out[j] = x;
    }
    cand_cnt[p] = n;
  }
}

__global__ __launch_bounds__(64) void logprob_finish_kernel(
    float* __restrict__ out_lp, int* __restrict__ out_top_id, float* __restrict__ out_top_lp,
    float* __restrict__ out_max, int* __restrict__ out_count, long long* __restrict__ out_mass,
    const unsigned long long* __restrict__ part_mass, const unsigned long long* __restrict__ cand,
    const int* __restrict__ cand_cnt, const uint32_t* __restrict__ part_key, const int* __restrict__ part_cnt,
    const bf16_t* __restrict__ logits, const uint32_t* __restrict__ mask_bits, const int* __restrict__ mask_idx,
    const int* __restrict__ token, int vocab, int mask_words, int vocab_offset, int top_n, int slices) {
  const int row = blockIdx.x, s = threadIdx.x;   // lane s = slice s (slices <= 64)
  const bool mine = s < slices;
  unsigned long long mass = mine ? part_mass[row * slices + s] : 0ull;
  int count = mine ? part_cnt[row * slices + s] : 0;
  uint32_t mk = mine ? part_key[row * slices + s] : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mass += shfl_xor_u64(mass, o);
    count += __shfl_xor(count, o, 64);
    mk = max(mk, (uint32_t)__shfl_xor((int)mk, o, 64));
  }
  const float m = count > 0 ? key_value(mk) : -INFINITY;
  const float log_s = logf((float)mass * INV_TWO40);
  // the n-way merge of the slices' sorted lists
  const int n_mine = (mine && top_n > 0) ? cand_cnt[row * slices + s] : 0;
  const unsigned long long* list = cand + (size_t)(row * slices + s) * top_n;
  int pos = 0;
  for (int j = 0; j < top_n; ++j) {
    const unsigned long long my = pos < n_mine ? list[pos] : SK_NONE;
    unsigned long long mn = my;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = shfl_xor_u64(mn, o);
      mn = other < mn ? other : mn;
    }
    if (mn != SK_NONE && my == mn) ++pos;   // ids are distinct: one lane holds the minimum
    if (s == 0) {
      if (mn == SK_NONE) {
        out_top_id[row * top_n + j] = -1;
        out_top_lp[row * top_n + j] = -INFINITY;
      } else {
        out_top_id[row * top_n + j] = (int)(uint32_t)mn + vocab_offset;
        out_top_lp[row * top_n + j] = (key_value(0xffffu - (uint32_t)(mn >> 32)) - m) - log_s;
      }
    }
  }
  if (s == 0) {
    float lp = -INFINITY;
    const int gid = token[row], i = gid - vocab_offset;
    if (count > 0 && i >= 0 && i < vocab) {
      const int mi = mask_idx ? mask_idx[row] : -1;
      const bool ok = mi < 0 || ((mask_bits[(size_t)mi * mask_words + (gid >> 5)] >> (gid & 31)) & 1u);
      if (ok) lp = (bf2f(logits[(size_t)row * vocab + i]) - m) - log_s;
    }
    out_lp[row] = lp;
    if (out_max) out_max[row] = m;
    if (out_count) out_count[row] = count;
    if (out_mass) out_mass[row] = (long long)mass;
  }
}

// workspace of ka_token_logprobs in 4-byte words (its base 8-byte aligned): per (row, slice) a sorted
// candidate list of top_n u64, the mass (u64), the largest key, the allowed count, the list length
extern "C" int ka_token_logprobs_ws_words(int rows, int slices, int top_n) {
  return rows * slices * (2 * top_n + 5);
}

// out_top_id / out_top_lp [rows, top_n] may be null when top_n == 0; out_max / out_count / out_mass may
// be null.  mask_bits null = no mask; with a mask, mask_words must cover the global ids
// [vocab_offset, vocab_offset + vocab).  token [rows]: global ids, read on the device.
extern "C" int ka_token_logprobs(float* out_lp, int* out_top_id, float* out_top_lp, float* out_max, int* out_count,
                                 void* out_mass, const void* logits, const uint32_t* mask_bits, const int* mask_idx,
                                 const int* token, int top_n, int rows, int vocab, int mask_words, int vocab_offset,
                                 void* workspace, int slices, hipStream_t stream) {
  if (rows <= 0) return 0;
  if (vocab <= 0 || vocab % 8 != 0 || vocab_offset % 8 != 0 || vocab_offset < 0 || slices < 1 || slices > 64 ||
      top_n < 0 || top_n > LP_MAX_TOP)
    return (int)hipErrorInvalidValue;
  if (out_lp == nullptr || logits == nullptr || token == nullptr || workspace == nullptr ||
      (top_n > 0 && (out_top_id == nullptr || out_top_lp == nullptr)))
    return (int)hipErrorInvalidValue;
  if (mask_bits != nullptr && (mask_idx == nullptr || (long long)mask_words * 32 < (long long)vocab_offset + vocab))
    return (int)hipErrorInvalidValue;
  const size_t rs = (size_t)rows * slices;
  unsigned long long* cand = static_cast<unsigned long long*>(workspace);
  unsigned long long* pmass = cand + rs * top_n;
  uint32_t* pkey = reinterpret_cast<uint32_t*>(pmass + rs);
  int* pcnt = reinterpret_cast<int*>(pkey + rs);
  int* ccnt = pcnt + rs;
  const bf16_t* lg = static_cast<const bf16_t*>(logits);
  const int* midx = mask_bits ? mask_idx : nullptr;
  hipLaunchKernelGGL(logprob_max_kernel, dim3(rows, slices), dim3(SAMPLE_NT), 0, stream, pkey, pcnt, lg, mask_bits,
                     midx, vocab, mask_words, vocab_offset);
  hipLaunchKernelGGL(logprob_slice_kernel, dim3(rows, slices), dim3(SAMPLE_NT), 0, stream, pmass, cand, ccnt, pkey,
                     pcnt, lg, mask_bits, midx, vocab, mask_words, vocab_offset, top_n);
  hipLaunchKernelGGL(logprob_finish_kernel, dim3(rows), dim3(64), 0, stream, out_lp, out_top_id, out_top_lp, out_max,
                     out_count, static_cast<long long*>(out_mass), pmass, cand, ccnt, pkey, pcnt, lg, mask_bits, midx,
                     token, vocab, mask_words, vocab_offset, top_n, slices);
  KA_CHECK_LAUNCH();
}
