// Row-scan helpers shared by the kernels that read a bf16 logit row under the SAFE_DECODE token mask
// with 512-thread workgroups: sampling_stochastic.hip (ka_sample) and logprobs.hip (ka_token_logprobs).
//   * bf16_key / key_value: the order-preserving 16-bit key of a bf16 pattern and back;
//   * scan_row: every allowed token of a row slice, each lane in increasing index order;
//   * Hist + hist_clear / hist_fold: one level (256 bins) of the exact two-level radix select on that
//     key, a count and a u64 fixed-point mass per bin, private to a wave and folded before each scan;
//   * block_argmax: largest (value, lowest index) of the workgroup.
#pragma once
#include "common.h"

constexpr int SAMPLE_NT = 512;
constexpr int SAMPLE_WAVES = SAMPLE_NT / 64;

// order-preserving 16-bit key of a bf16 pattern (larger value <=> larger key); -0 counts as +0
KA_DEV uint32_t bf16_key(uint32_t b) {
  b = b == 0x8000u ? 0u : b;
  return (b & 0x8000u) ? (b ^ 0xffffu) : (b | 0x8000u);
}
KA_DEV float key_value(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (k ^ 0xffffu);
  return __uint_as_float(b << 16);
}

// f(local index, bf16 pattern, value) for every allowed token of vectors [v0, nvec) of a row, each
// lane in increasing index order.  Batches of UN vectors per lane, as in masked_argmax_kernel: the
// UN mask words are issued together, then the logits of the vectors with any bit set, then all are
// scanned (one vector per iteration would wait for its mask word and then for its logits).
template <typename F>
KA_DEV void scan_row(const bf16_t* __restrict__ lr, const uint32_t* __restrict__ mrow, int v0, int nvec,
                     int vocab_offset, F&& f) {
  constexpr int UN = 8;
  for (int v = v0 + threadIdx.x; v < nvec; v += SAMPLE_NT * UN) {
    uint32_t bits[UN], raw[UN];
    uint4 q[UN];
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int gb = ((v + j * SAMPLE_NT) << 3) + vocab_offset;   // the mask is indexed by the global token id
      raw[j] = 0xffffffffu;
      if (mrow && v + j * SAMPLE_NT < nvec) raw[j] = mrow[gb >> 5];
    }
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      const int gb = ((v + j * SAMPLE_NT) << 3) + vocab_offset;
      bits[j] = v + j * SAMPLE_NT < nvec ? (mrow ? (raw[j] >> (gb & 31)) & 0xffu : 0xffu) : 0u;
      if (bits[j]) q[j] = *reinterpret_cast<const uint4*>(lr + ((v + j * SAMPLE_NT) << 3));
    }
#pragma unroll
    for (int j = 0; j < UN; ++j) {
      if (!bits[j]) continue;
      const int base = (v + j * SAMPLE_NT) << 3;
      const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t b = (k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu);
        if ((bits[j] >> k) & 1u) f(base + k, b, __uint_as_float(b << 16));
      }
    }
  }
}

struct Hist {
  uint32_t cnt[SAMPLE_WAVES][256];
  unsigned long long mass[SAMPLE_WAVES][256];
};

KA_DEV void hist_clear(Hist& h) {
  for (int i = threadIdx.x; i < SAMPLE_WAVES * 256; i += SAMPLE_NT) {
    (&h.cnt[0][0])[i] = 0u;
    (&h.mass[0][0])[i] = 0ull;
  }
  __syncthreads();
}

// fold the waves' private bins into copy 0 (after the barrier that ends the pass)
KA_DEV void hist_fold(Hist& h) {
  __syncthreads();
  if (threadIdx.x < 256) {
    uint32_t c = 0u;
    unsigned long long m = 0ull;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) {
      c += h.cnt[w][threadIdx.x];
      m += h.mass[w][threadIdx.x];
    }
    h.cnt[0][threadIdx.x] = c;
    h.mass[0][threadIdx.x] = m;
  }
  __syncthreads();
}

// largest (value, lowest index) of the workgroup, in thread 0
KA_DEV void block_argmax(float& best, int& bidx, float* sb, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bidx, o, 64);
    if (ob > best || (ob == best && oi < bidx)) {
      best = ob;
      bidx = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sb[threadIdx.x >> 6] = best;
    si[threadIdx.x >> 6] = bidx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    best = sb[0];
    bidx = si[0];
    for (int i = 1; i < SAMPLE_WAVES; ++i)
      if (sb[i] > best || (sb[i] == best && si[i] < bidx)) {
        best = sb[i];
        bidx = si[i];
      }
  }
}
