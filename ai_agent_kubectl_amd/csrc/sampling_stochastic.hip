// Seeded temperature / top-k / top-p sampling under the SAFE_DECODE token mask, by Gumbel-max.
//
// A draw from softmax(l / T) is argmax_i (l_i / T + g_i) with g_i = -log(-log(u_i)) Gumbel noise.
// u_i is a pure function of (seed, position, GLOBAL token id) (splitmix64, gumbel_u below), so sampling
// has the shape of the greedy sampler in sampling.hip: one argmax per row, ties to the lowest id, a
// (score, global id) pair per row that argmax_combine merges across vocab-parallel ranks, and a token
// that does not depend on the batch the request rode in.
//
// Per row (A = tokens the mask allows, l_i = the bf16 logit as fp32):
//   * temperature == 0: the masked argmax of sampling.hip, bit for bit (top_k / top_p / seed ignored);
//   * top_k = k > 0: tau_k = the min(k, |A|)-th largest l_i over A (duplicates counted); keep l_i >= tau_k
//     (ties at the cut stay);
//   * top_p = p < 1, after top-k: w_i = exp((l_i - m) / T) over the kept set (m = its maximum); walking
//     the distinct logit values downwards, tau_p = the first value at which mass{l_i >= tau_p} reaches
//     p x the total mass; keep l_i >= tau_p;
//   * the token = argmax over the kept set of l_i / T + g_i in fp32, the lowest id on ties.
//
// A bf16 logit has 65,536 possible values, so both cuts are an exact two-level radix select on the
// order-preserving 16-bit key of the bf16 pattern: 256 LDS bins on the high byte, then 256 on the low
// byte inside the chosen bin, each with a count (top-k) and a mass (top-p).  Masses are summed as u64
// fixed point (w x 2^40, truncated; a 128k-entry row of weights <= 1 stays below 2^57): integer sums
// do not depend on the order of the atomics, so the cut — and the token — is the same in every run.
// Bins are private to a wave (8 copies), folded before each scan.
//
// Grid rows x slices like masked_argmax_kernel.  A row without an active cut is one pass and is cut
// into slices; a row with a cut is worked by its slice-0 workgroup alone (the other slices report
// nothing), up to five passes over a row that stays in L2.  sample_finish_kernel picks the winner of
// the slices' partials, as argmax_finish_kernel does for the argmax.
#include "sampling_common.h"

namespace {

constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ull;

KA_DEV unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// u in (0, 1): (2 * (z >> 41) + 1) * 2^-24 is an odd multiple of 2^-24 below 1, exact in fp32
KA_DEV float gumbel_u(unsigned long long key, int gid) {
  const unsigned long long z = mix64(key + (unsigned long long)(gid + 1) * GOLDEN);
  return (float)(2u * (uint32_t)(z >> 41) + 1u) * 5.9604644775390625e-08f;
}

// logf, not __logf: the tests' score margin is derived from logf's accuracy
KA_DEV float gumbel(float u) { return -logf(-logf(u)); }

}  // namespace

__global__ __launch_bounds__(SAMPLE_NT) void sample_kernel(
    int* __restrict__ out_idx, float* __restrict__ out_val, float* __restrict__ out_cut, int* __restrict__ out_kept,
    const bf16_t* __restrict__ logits, const uint32_t* __restrict__ mask_bits, const int* __restrict__ mask_idx,
    const float* __restrict__ temperature, const int* __restrict__ top_k, const float* __restrict__ top_p,
    const unsigned long long* __restrict__ seed, const int* __restrict__ position, int vocab, int mask_words,
    int vocab_offset, float* __restrict__ part_val, int* __restrict__ part_idx, int* __restrict__ part_cnt,
    float* __restrict__ part_cut) {
  __shared__ Hist hist;
  __shared__ float sb[SAMPLE_WAVES];
  __shared__ int si[SAMPLE_WAVES];
  __shared__ int s_sel[4];   // scan results: [bin, count above the bin, kept count] (+ pad)
  __shared__ unsigned long long s_mass[2];   // [mass above the chosen bin, total mass]

  const int row = blockIdx.x;
  const bf16_t* lr = logits + (size_t)row * vocab;
  const int mi = mask_idx ? mask_idx[row] : -1;
  const uint32_t* mrow = mi >= 0 ? mask_bits + (size_t)mi * mask_words : nullptr;
  const float T = temperature[row];
  const bool greedy = !(T > 0.f);
  const int k_req = greedy ? 0 : top_k[row];
  const float p_req = greedy ? 1.f : top_p[row];
  const bool cuts = k_req > 0 || p_req < 1.f;
  const unsigned long long key =
      greedy ? 0ull : mix64(seed[row] + (unsigned long long)((long long)position[row] + 1) * GOLDEN);
  const int wave = threadIdx.x >> 6;

  const int nvec_all = vocab >> 3;
  int v0 = 0, nvec = nvec_all;
  if (!cuts) {   // one pass: sliced like the argmax
    const int per = (nvec_all + gridDim.y - 1) / gridDim.y;
    v0 = blockIdx.y * per;
    nvec = min(nvec_all, v0 + per);
  } else if (blockIdx.y != 0) {
    nvec = 0;    // a row with a cut is its slice-0 workgroup's: this slice reports nothing
  }

  uint32_t cut_key = 0u;   // keep key >= cut_key
  int kept = 0;
  if (cuts && nvec > 0) {
    // ---- pass 1: counts per high byte over A ----
    hist_clear(hist);
    scan_row(lr, mrow, v0, nvec, vocab_offset,
             [&](int, uint32_t b, float) { atomicAdd(&hist.cnt[wave][bf16_key(b) >> 8], 1u); });
    hist_fold(hist);
    if (threadIdx.x == 0) {
      int total = 0;
      for (int i = 0; i < 256; ++i) total += (int)hist.cnt[0][i];
      const int k = k_req > 0 ? min(k_req, total) : total;   // k >= |A| (or top-k off): keep A
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
      s_sel[3] = total;
    }
    __syncthreads();
    const int total = s_sel[3];
    if (total > 0) {
      // ---- pass 2: counts per low byte inside the chosen bin -> tau_k ----
      const uint32_t hb = (uint32_t)s_sel[0];
      const int above_k = s_sel[1], k = s_sel[2];
      hist_clear(hist);
      scan_row(lr, mrow, v0, nvec, vocab_offset, [&](int, uint32_t b, float) {
        const uint32_t ky = bf16_key(b);
        if ((ky >> 8) == hb) atomicAdd(&hist.cnt[wave][ky & 0xffu], 1u);
      });
      hist_fold(hist);
      if (threadIdx.x == 0) {
        int cum = above_k, lo = 0;
        for (int i = 255; i >= 0; --i) {
          cum += (int)hist.cnt[0][i];
          if (hist.cnt[0][i] > 0 && cum >= k) {
            lo = i;
            break;
          }
        }
        s_sel[0] = (int)((hb << 8) | (uint32_t)lo);
        s_sel[1] = cum;
      }
      __syncthreads();
      cut_key = (uint32_t)s_sel[0];
      kept = s_sel[1];
      __syncthreads();
      if (p_req < 1.f) {
        // ---- the kept set's maximum (the row's: top-k keeps it) ----
        uint32_t mk = 0u;
        scan_row(lr, mrow, v0, nvec, vocab_offset, [&](int, uint32_t b, float) { mk = max(mk, bf16_key(b)); });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mk = max(mk, (uint32_t)__shfl_xor((int)mk, o, 64));
        if ((threadIdx.x & 63) == 0) si[wave] = (int)mk;
        __syncthreads();
        for (int i = 0; i < SAMPLE_WAVES; ++i) mk = max(mk, (uint32_t)si[i]);
        const float m = key_value(mk);
        const uint32_t tk = cut_key;
        // ---- pass 3: mass and count per high byte over the top-k set ----
        hist_clear(hist);
        scan_row(lr, mrow, v0, nvec, vocab_offset, [&](int, uint32_t b, float x) {
          const uint32_t ky = bf16_key(b);
          if (ky < tk) return;
          const float w = expf((x - m) / T);
          atomicAdd(&hist.cnt[wave][ky >> 8], 1u);
          atomicAdd(&hist.mass[wave][ky >> 8], (unsigned long long)(w * 1099511627776.f));
        });
        hist_fold(hist);
        if (threadIdx.x == 0) {
          unsigned long long tot = 0ull;
          for (int i = 0; i < 256; ++i) tot += hist.mass[0][i];
          const double target = (double)p_req * (double)tot;
          unsigned long long cum = 0ull;
          int cnt = 0, bin = (int)(tk >> 8);
          for (int i = 255; i >= (int)(tk >> 8); --i) {
            if (hist.cnt[0][i] > 0 && (double)(cum + hist.mass[0][i]) >= target) {
              bin = i;
              break;
            }
            cum += hist.mass[0][i];
            cnt += (int)hist.cnt[0][i];
          }
          s_sel[0] = bin;
          s_sel[1] = cnt;
          s_mass[0] = cum;
          s_mass[1] = tot;
        }
        __syncthreads();
        const uint32_t pb = (uint32_t)s_sel[0];
        const int above_p = s_sel[1];
        const unsigned long long mass_above = s_mass[0], mass_total = s_mass[1];
        // ---- pass 4: mass and count per low byte inside the chosen bin -> tau_p ----
        hist_clear(hist);
        scan_row(lr, mrow, v0, nvec, vocab_offset, [&](int, uint32_t b, float x) {
          const uint32_t ky = bf16_key(b);
          if (ky < tk || (ky >> 8) != pb) return;
          const float w = expf((x - m) / T);
          atomicAdd(&hist.cnt[wave][ky & 0xffu], 1u);
          atomicAdd(&hist.mass[wave][ky & 0xffu], (unsigned long long)(w * 1099511627776.f));
        });
        hist_fold(hist);
        if (threadIdx.x == 0) {
          const double target = (double)p_req * (double)mass_total;
          const int lo_min = (pb == (tk >> 8)) ? (int)(tk & 0xffu) : 0;
          unsigned long long cum = mass_above;
          int cnt = above_p, lo = lo_min;
          for (int i = 255; i >= lo_min; --i) {
            cum += hist.mass[0][i];
            cnt += (int)hist.cnt[0][i];
            if (hist.cnt[0][i] > 0 && (double)cum >= target) {
              lo = i;
              break;
            }
          }
          s_sel[0] = (int)((pb << 8) | (uint32_t)lo);
          s_sel[1] = cnt;
        }
        __syncthreads();
        cut_key = (uint32_t)s_sel[0];
        kept = s_sel[1];
        __syncthreads();
      }
    }
  }

  // ---- the draw (or the greedy argmax): one pass over the kept set ----
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  int cnt = 0;
  if (greedy) {
    scan_row(lr, mrow, v0, nvec, vocab_offset, [&](int i, uint32_t, float x) {
      ++cnt;
      if (x > best) {   // strict '>' keeps the lowest index within a lane
        best = x;
        bidx = i;
      }
    });
  } else {
    const uint32_t ck = cut_key;
    scan_row(lr, mrow, v0, nvec, vocab_offset, [&](int i, uint32_t b, float x) {
      ++cnt;
      if (bf16_key(b) < ck) return;
      const float s = x / T + gumbel(gumbel_u(key, i + vocab_offset));
      if (s > best) {
        best = s;
        bidx = i;
      }
    });
  }
  block_argmax(best, bidx, sb, si);
  if (!cuts) {   // no cut: every allowed token is kept
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) si[wave] = cnt;
    __syncthreads();
    kept = 0;
    for (int i = 0; i < SAMPLE_WAVES; ++i) kept += si[i];
  }
  if (threadIdx.x == 0) {
    const float cut = cuts && nvec > 0 && s_sel[3] > 0 ? key_value(cut_key) : -INFINITY;
    if (part_val != nullptr) {   // sliced launch: the finish kernel decides
      const int p = row * gridDim.y + blockIdx.y;
      part_val[p] = best;
      part_idx[p] = bidx;
      part_cnt[p] = kept;
      if (blockIdx.y == 0) part_cut[row] = cut;
      return;
    }
    if (bidx == 0x7fffffff) bidx = 0;  // fully masked row (cannot happen with a valid mask): token 0
    out_idx[row] = bidx + vocab_offset;
    if (out_val) out_val[row] = best;
    if (out_cut) out_cut[row] = cut;
    if (out_kept) out_kept[row] = kept;
  }
}

__global__ __launch_bounds__(64) void sample_finish_kernel(int* __restrict__ out_idx, float* __restrict__ out_val,
                                                           float* __restrict__ out_cut, int* __restrict__ out_kept,
                                                           const float* __restrict__ part_val,
                                                           const int* __restrict__ part_idx,
                                                           const int* __restrict__ part_cnt,
                                                           const float* __restrict__ part_cut, int slices,
                                                           int vocab_offset) {
  const int row = blockIdx.x;
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  int kept = 0;
  for (int i = threadIdx.x; i < slices; i += 64) {
    const float v = part_val[row * slices + i];
    const int ix = part_idx[row * slices + i];
    kept += part_cnt[row * slices + i];
    if (v > best || (v == best && ix < bidx)) {
      best = v;
      bidx = ix;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bidx, o, 64);
    kept += __shfl_xor(kept, o, 64);
    if (ob > best || (ob == best && oi < bidx)) {
      best = ob;
      bidx = oi;
    }
  }
  if (threadIdx.x == 0) {
    if (bidx == 0x7fffffff) bidx = 0;
    out_idx[row] = bidx + vocab_offset;
    if (out_val) out_val[row] = best;
    if (out_cut) out_cut[row] = part_cut[row];
    if (out_kept) out_kept[row] = kept;
  }
}

// slices > 1 needs a workspace of ka_sample_ws_words(rows, slices) 4-byte words.
extern "C" int ka_sample_ws_words(int rows, int slices) { return slices > 1 ? rows * slices * 3 + rows : 0; }

// out_cut / out_kept may be null.  mask_bits null = no mask; with a mask, mask_words must cover the
// global ids [vocab_offset, vocab_offset + vocab).
extern "C" int ka_sample(int* out_idx, float* out_val, float* out_cut, int* out_kept, const void* logits,
                         const uint32_t* mask_bits, const int* mask_idx, const float* temperature, const int* top_k,
                         const float* top_p, const void* seed, const int* position, int rows, int vocab,
                         int mask_words, int vocab_offset, void* workspace, int slices, hipStream_t stream) {
  if (rows <= 0) return 0;
  if (vocab % 8 != 0 || vocab_offset % 8 != 0 || vocab_offset < 0 || slices < 1 ||
      (slices > 1 && workspace == nullptr))
    return (int)hipErrorInvalidValue;
  if (out_idx == nullptr || logits == nullptr || temperature == nullptr || top_k == nullptr || top_p == nullptr ||
      seed == nullptr || position == nullptr)
    return (int)hipErrorInvalidValue;
  if (mask_bits != nullptr && (mask_idx == nullptr || (long long)mask_words * 32 < (long long)vocab_offset + vocab))
    return (int)hipErrorInvalidValue;
  float* pv = slices > 1 ? static_cast<float*>(workspace) : nullptr;
  int* pi = slices > 1 ? reinterpret_cast<int*>(pv + (size_t)rows * slices) : nullptr;
  int* pc = slices > 1 ? pi + (size_t)rows * slices : nullptr;
  float* pcut = slices > 1 ? reinterpret_cast<float*>(pc + (size_t)rows * slices) : nullptr;
  hipLaunchKernelGGL(sample_kernel, dim3(rows, slices), dim3(SAMPLE_NT), 0, stream, out_idx, out_val, out_cut,
                     out_kept, static_cast<const bf16_t*>(logits), mask_bits, mask_bits ? mask_idx : nullptr,
                     temperature, top_k, top_p, static_cast<const unsigned long long*>(seed), position, vocab,
                     mask_words, vocab_offset, pv, pi, pc, pcut);
  if (slices > 1)
    hipLaunchKernelGGL(sample_finish_kernel, dim3(rows), dim3(64), 0, stream, out_idx, out_val, out_cut, out_kept,
                       pv, pi, pc, pcut, slices, vocab_offset);
  KA_CHECK_LAUNCH();
}
