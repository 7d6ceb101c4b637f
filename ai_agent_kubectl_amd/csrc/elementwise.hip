// Memory-bound kernels: fused residual-add + RMSNorm (K2), neox RoPE fused with the paged-KV append
// (K4), SiLU*mul (K8 epilogue), embedding gather (K1).  All bf16 I/O is 16 B per lane.
//
// Layouts (shared with attention.hip and the torch references in ops/reference.py):
//   qkv      [T, (Hq + 2*Hkv) * D]   output of the fused QKV projection
//   cos_sin  [max_pos, D] f32        cos in [0, D/2), sin in [D/2, D) (host-precomputed, guide App. B)
//   k_cache  [NB, Hkv, BS, D]        token-major blocks: a 16-token K block is one 4 KiB run
//   v_cache  [NB, Hkv, D, BS]        dim-major blocks: 8 consecutive tokens of one dim are 16 B, which
//                                    is exactly the B-operand fragment of the P*V MFMA
//   slot_mapping[t] = block * BS + offset, or -1 for padding tokens (no cache write).
#include "common.h"

// ------------------------------------------------------------------------------------------------
// RMSNorm, optionally fused with the residual add:   r = x (+ residual);  residual = r;
//                                                  out = r * rsqrt(mean(r^2) + eps) * w
// and optionally with the split-K reduction of the GEMM that produced x: x = bf16(sum_k P[k]) where P
// holds `split` fp32 partial slabs of [rows, hidden] (gemm_skinny / gemm_mfma with no output), so
// the projection's reduce kernel and its bf16 round trip through HBM disappear.
// PT: element type of the split-K slices P (float, or bf16_t from gemm_mfma EPI_P16).
//
// Every load a thread needs (its split-K slices, the residual, the norm weight) is issued before the
// first use: up to UNR slices unrolled, further slices UNR at a time.  A rolled slice loop
// waited for each slice before issuing the next, so a split-4 norm paid ~6 serial memory latencies.
// The slices are still summed in order k = 0, 1, ... (bitwise the old result).
struct f32x8_raw {
  f32x4 a, b;
};
template <typename PT, typename Raw>
KA_DEV void unpack_part8(const Raw& r, f32x4& s0, f32x4& s1) {
  if constexpr (sizeof(PT) == 4) {
    s0 = r.a;
    s1 = r.b;
  } else {
    s0 = f32x4{lo_f(r.x), hi_f(r.x), lo_f(r.y), hi_f(r.y)};
    s1 = f32x4{lo_f(r.z), hi_f(r.z), lo_f(r.w), hi_f(r.w)};
  }
}

template <int NT, int MAXV, typename PT = float>
__global__ __launch_bounds__(NT) void rmsnorm_kernel(bf16_t* __restrict__ out, bf16_t* __restrict__ residual,
                                                     const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                     int hidden, float eps, const PT* __restrict__ P, int split,
                                                     size_t pstride) {
  constexpr int UNR = MAXV == 1 ? (NT >= 512 ? 8 : 4) : (MAXV == 2 ? 4 : 2);
  const int row = blockIdx.x;
  const int nvec = hidden >> 3;
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * hidden);
  uint4* rr = residual ? reinterpret_cast<uint4*>(residual + (size_t)row * hidden) : nullptr;
  const uint4* wr = reinterpret_cast<const uint4*>(w);
  float v[MAXV][8];
  uint4 g[MAXV];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      uint4 a, b = make_uint4(0u, 0u, 0u, 0u);
      g[i] = wr[idx];
      if (P != nullptr) {
        const PT* pr = P + (size_t)row * hidden + idx * 8;
        // raw loads first (the unpack of a bf16 slice next to its load would wait for it right there)
        using Raw = typename std::conditional<sizeof(PT) == 4, f32x8_raw, uint4>::type;
        Raw t[UNR];
#pragma unroll
        for (int k = 0; k < UNR; ++k)
          if (k == 0 || k < split) t[k] = *reinterpret_cast<const Raw*>(pr + k * pstride);
        if (rr) b = rr[idx];
        f32x4 s0, s1;
        unpack_part8<PT>(t[0], s0, s1);
#pragma unroll
        for (int k = 1; k < UNR; ++k) {
          if (k < split) {
            f32x4 u0, u1;
            unpack_part8<PT>(t[k], u0, u1);
            s0 += u0;
            s1 += u1;
          }
        }
        for (int k0 = UNR; k0 < split; k0 += UNR) {   // further slices, UNR loads per wait
#pragma unroll
          for (int k = 0; k < UNR; ++k)
            if (k0 + k < split) t[k] = *reinterpret_cast<const Raw*>(pr + (k0 + k) * pstride);
#pragma unroll
          for (int k = 0; k < UNR; ++k) {
            if (k0 + k < split) {
              f32x4 u0, u1;
              unpack_part8<PT>(t[k], u0, u1);
              s0 += u0;
              s1 += u1;
            }
          }
        }
        a = make_uint4(pack2(s0[0], s0[1]), pack2(s0[2], s0[3]), pack2(s1[0], s1[1]), pack2(s1[2], s1[3]));
      } else {
        a = xr[idx];
        if (rr) b = rr[idx];
      }
      uint32_t aw[4] = {a.x, a.y, a.z, a.w};
      if (rr) {
        uint32_t bw[4] = {b.x, b.y, b.z, b.w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // round the sum to bf16 first: the residual stream is stored in bf16
          float s0 = bf2f(f2bf(lo_f(aw[k]) + lo_f(bw[k])));
          float s1 = bf2f(f2bf(hi_f(aw[k]) + hi_f(bw[k])));
          v[i][2 * k] = s0;
          v[i][2 * k + 1] = s1;
          o[k] = pack2(s0, s1);
        }
        rr[idx] = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[i][2 * k] = lo_f(aw[k]);
          v[i][2 * k + 1] = hi_f(aw[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) ss += v[i][k] * v[i][k];
    }
  }
  __shared__ float red[NT / 64];
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) tot += red[i];
  const float scale = rsqrtf(tot / (float)hidden + eps);
  uint4* orow = reinterpret_cast<uint4*>(out + (size_t)row * hidden);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int idx = threadIdx.x + i * NT;
    if (idx < nvec) {
      uint32_t gw[4] = {g[i].x, g[i].y, g[i].z, g[i].w};
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = pack2(v[i][2 * k] * scale * lo_f(gw[k]), v[i][2 * k + 1] * scale * hi_f(gw[k]));
      orow[idx] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

extern "C" int ka_rmsnorm(void* out, void* residual, const void* x, const void* w, int rows, int hidden,
                          float eps, hipStream_t stream) {
  if (rows <= 0) return 0;
  if (hidden % 8 != 0 || hidden > 256 * 8 * 4) return (int)hipErrorInvalidValue;
  const int nvec = hidden / 8;
  auto* o = static_cast<bf16_t*>(out);
  auto* r = static_cast<bf16_t*>(residual);
  auto* xi = static_cast<const bf16_t*>(x);
  auto* wi = static_cast<const bf16_t*>(w);
  const float* P = nullptr;
  const int split = 0;
  const size_t pstride = 0;
  if (nvec <= 256)
    hipLaunchKernelGGL((rmsnorm_kernel<256, 1>), dim3(rows), dim3(256), 0, stream, o, r, xi, wi, hidden, eps, P,
                       split, pstride);
  else if (nvec <= 512 && rows <= 1024)   // decode-sized: one 16-B vector per thread, 8 waves per row
    hipLaunchKernelGGL((rmsnorm_kernel<512, 1>), dim3(rows), dim3(512), 0, stream, o, r, xi, wi, hidden, eps, P,
                       split, pstride);
  else if (nvec <= 512)
    hipLaunchKernelGGL((rmsnorm_kernel<256, 2>), dim3(rows), dim3(256), 0, stream, o, r, xi, wi, hidden, eps, P,
                       split, pstride);
  else
    hipLaunchKernelGGL((rmsnorm_kernel<256, 4>), dim3(rows), dim3(256), 0, stream, o, r, xi, wi, hidden, eps, P,
                       split, pstride);
  KA_CHECK_LAUNCH();
}

template <typename PT>
static void launch_rmsnorm_splitk(bf16_t* o, bf16_t* r, const PT* p, int split, const bf16_t* wi, int rows, int hidden,
                                  float eps, hipStream_t stream) {
  const int nvec = hidden / 8;
  const size_t ps = (size_t)rows * hidden;
  if (nvec <= 256)
    hipLaunchKernelGGL((rmsnorm_kernel<256, 1, PT>), dim3(rows), dim3(256), 0, stream, o, r, nullptr, wi, hidden, eps,
                       p, split, ps);
  else if (nvec <= 512)   // the split slabs are read once: 8 waves per row keep more loads in flight
    hipLaunchKernelGGL((rmsnorm_kernel<512, 1, PT>), dim3(rows), dim3(512), 0, stream, o, r, nullptr, wi, hidden, eps,
                       p, split, ps);
  else if (nvec <= 1024 && rows <= 1024)   // hidden 8192 at decode sizes: 8 waves, 4 slices per batch
    hipLaunchKernelGGL((rmsnorm_kernel<512, 2, PT>), dim3(rows), dim3(512), 0, stream, o, r, nullptr, wi, hidden, eps,
                       p, split, ps);
  else
    hipLaunchKernelGGL((rmsnorm_kernel<256, 4, PT>), dim3(rows), dim3(256), 0, stream, o, r, nullptr, wi, hidden, eps,
                       p, split, ps);
}

// out = rmsnorm(bf16(sum_k P[k]) (+ residual)) * w; P = split slabs of [rows, hidden], fp32 or (p_bf16) bf16
extern "C" int ka_rmsnorm_splitk(void* out, void* residual, const void* P, int split, int p_bf16, const void* w,
                                 int rows, int hidden, float eps, hipStream_t stream) {
  if (rows <= 0) return 0;
  if (hidden % 8 != 0 || hidden > 256 * 8 * 4 || split < 1) return (int)hipErrorInvalidValue;
  auto* o = static_cast<bf16_t*>(out);
  auto* r = static_cast<bf16_t*>(residual);
  auto* wi = static_cast<const bf16_t*>(w);
  if (p_bf16)
    launch_rmsnorm_splitk(o, r, static_cast<const bf16_t*>(P), split, wi, rows, hidden, eps, stream);
  else
    launch_rmsnorm_splitk(o, r, static_cast<const float*>(P), split, wi, rows, hidden, eps, stream);
  KA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------
// RoPE (neox / rotate-half pairs (i, i + D/2)) on q and k, q -> q_out [T, Hq, D], k and v -> paged cache.
// With P != nullptr the qkv row is the bf16-rounded sum of `split` fp32 split-K partial slabs of the
// QKV projection (bit-identical to splitk_reduce_kernel + this kernel, one launch and HBM pass fewer).
// The split-K slices are loaded SK_BATCH at a time, each batch issued before its first add (a rolled
// loop waited for every slice before issuing the next); summed in order k = 0, 1, ...  N reads
// (e.g. the gate and up halves of silu_mul) share each batch.
constexpr int SK_BATCH = 4;
template <int N>
__device__ __forceinline__ void sum8_slices(const float* P, int split, size_t pstride, const size_t (&off)[N],
                                            f32x4 (&lo)[N], f32x4 (&hi)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) lo[n] = hi[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < split; k0 += SK_BATCH) {
    f32x4 a[SK_BATCH][N], b[SK_BATCH][N];
#pragma unroll
    for (int k = 0; k < SK_BATCH; ++k)
#pragma unroll
      for (int n = 0; n < N; ++n)
        if (k0 + k < split) {
          a[k][n] = *reinterpret_cast<const f32x4*>(P + (k0 + k) * pstride + off[n]);
          b[k][n] = *reinterpret_cast<const f32x4*>(P + (k0 + k) * pstride + off[n] + 4);
        }
#pragma unroll
    for (int k = 0; k < SK_BATCH; ++k)
#pragma unroll
      for (int n = 0; n < N; ++n)
        if (k0 + k < split) {
          lo[n] += a[k][n];
          hi[n] += b[k][n];
        }
  }
}

__device__ __forceinline__ uint2 ld4(const bf16_t* row, const float* P, int split, size_t pstride, size_t off) {
  if (P == nullptr) return *reinterpret_cast<const uint2*>(row + off);
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < split; k0 += SK_BATCH) {
    f32x4 a[SK_BATCH];
#pragma unroll
    for (int k = 0; k < SK_BATCH; ++k)
      if (k0 + k < split) a[k] = *reinterpret_cast<const f32x4*>(P + (k0 + k) * pstride + off);
#pragma unroll
    for (int k = 0; k < SK_BATCH; ++k)
      if (k0 + k < split) s += a[k];
  }
  return make_uint2(pack2(s[0], s[1]), pack2(s[2], s[3]));
}

__device__ __forceinline__ uint4 ld8(const bf16_t* row, const float* P, int split, size_t pstride, size_t off) {
  if (P == nullptr) return *reinterpret_cast<const uint4*>(row + off);
  const size_t o[1] = {off};
  f32x4 lo[1], hi[1];
  sum8_slices<1>(P, split, pstride, o, lo, hi);
  return make_uint4(pack2(lo[0][0], lo[0][1]), pack2(lo[0][2], lo[0][3]), pack2(hi[0][0], hi[0][1]),
                    pack2(hi[0][2], hi[0][3]));
}

__global__ __launch_bounds__(256) void rope_kv_kernel(bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_cache,
                                                      bf16_t* __restrict__ v_cache, const bf16_t* __restrict__ qkv,
                                                      const int* __restrict__ positions,
                                                      const float* __restrict__ cos_sin,
                                                      const int* __restrict__ slot_mapping, int hq, int hkv, int d,
                                                      int bs, const float* __restrict__ Pq, int split,
                                                      size_t pstride) {
  const int t = blockIdx.x;
  const int half = d >> 1;
  const int qkv_stride = (hq + 2 * hkv) * d;
  const bf16_t* row = qkv + (size_t)t * qkv_stride;
  const float* prow = Pq ? Pq + (size_t)t * qkv_stride : nullptr;
  const int pos = positions[t];
  const int slot = slot_mapping[t];
  const float* cs = cos_sin + (size_t)pos * d;
  const int chunks = half >> 2;  // 4 pairs per item
  const int n_rot = (hq + hkv) * chunks;
  const int blk = slot >= 0 ? slot / bs : 0;
  const int off = slot >= 0 ? slot % bs : 0;
  for (int it = threadIdx.x; it < n_rot; it += blockDim.x) {
    const int h = it / chunks;
    const int i = (it % chunks) * 4;
    // q heads first, then k heads (contiguous in qkv)
    uint2 a = ld4(row, prow, split, pstride, (size_t)h * d + i);
    uint2 b = ld4(row, prow, split, pstride, (size_t)h * d + i + half);
    float4 c = *reinterpret_cast<const float4*>(cs + i);
    float4 s = *reinterpret_cast<const float4*>(cs + half + i);
    float x1[4] = {lo_f(a.x), hi_f(a.x), lo_f(a.y), hi_f(a.y)};
    float x2[4] = {lo_f(b.x), hi_f(b.x), lo_f(b.y), hi_f(b.y)};
    float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {s.x, s.y, s.z, s.w};
    float o1[4], o2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o1[k] = x1[k] * cc[k] - x2[k] * ss[k];
      o2[k] = x2[k] * cc[k] + x1[k] * ss[k];
    }
    uint2 r1 = make_uint2(pack2(o1[0], o1[1]), pack2(o1[2], o1[3]));
    uint2 r2 = make_uint2(pack2(o2[0], o2[1]), pack2(o2[2], o2[3]));
    bf16_t* dst;
    if (h < hq) {
      dst = q_out + ((size_t)t * hq + h) * d;
    } else {
      if (slot < 0) continue;
      dst = k_cache + (((size_t)blk * hkv + (h - hq)) * bs + off) * d;
    }
    *reinterpret_cast<uint2*>(dst + i) = r1;
    *reinterpret_cast<uint2*>(dst + i + half) = r2;
  }
  if (slot < 0) return;
  const int vchunks = d >> 3;
  const size_t vbase = (size_t)(hq + hkv) * d;
  for (int it = threadIdx.x; it < hkv * vchunks; it += blockDim.x) {
    const int h = it / vchunks;
    const int i = (it % vchunks) * 8;
    uint4 v = ld8(row, prow, split, pstride, vbase + (size_t)h * d + i);
    bf16_t e[8] = {(bf16_t)v.x, (bf16_t)(v.x >> 16), (bf16_t)v.y, (bf16_t)(v.y >> 16),
                   (bf16_t)v.z, (bf16_t)(v.z >> 16), (bf16_t)v.w, (bf16_t)(v.w >> 16)};
    bf16_t* dst = v_cache + (((size_t)blk * hkv + h) * d + i) * bs + off;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[(size_t)k * bs] = e[k];
  }
}

// Prefill-sized RoPE + KV append: one workgroup per window of 16 consecutive tokens.  The per-token
// kernel above writes the dim-major V cache ([blk][h][d][16]) as isolated 2-byte stores, one per
// (token, dim), each to its own 32-byte segment — the write path, not the math, bounded it (~3x the
// q/k/v bytes at 6 TB/s).  Here each head's 16 x 128 V tile is loaded with 16-B loads, transposed
// through LDS, and stored with lanes = the 16 tokens of one dim, so the 16 stores of a wave quarter
// hit consecutive addresses whenever the tokens' slots are consecutive (one 32-B segment per dim for
// a block-aligned window, two when it straddles a block boundary).
__global__ __launch_bounds__(256) void rope_kv_window_kernel(bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_cache,
                                                             bf16_t* __restrict__ v_cache,
                                                             const bf16_t* __restrict__ qkv,
                                                             const int* __restrict__ positions,
                                                             const float* __restrict__ cos_sin,
                                                             const int* __restrict__ slot_mapping, int tokens, int hq,
                                                             int hkv, const float* __restrict__ Pq, int split,
                                                             size_t pstride) {
  constexpr int d = 128, half = 64, bs = 16, W = 16;
  __shared__ bf16_t vt[d][W + 2];   // [dim][token] (+2 pad: the transposing writes spread over banks)
  const int t0 = blockIdx.x * W;
  const int nt = min(W, tokens - t0);
  const int qkv_stride = (hq + 2 * hkv) * d;
  // ---- q / k rotation: (hq + hkv) heads x 8 items of 8 rotary pairs per token, 16-B loads and
  // stores.  The window's slots and positions are staged in LDS first, so no item's loads wait for a
  // global read of its token's slot / position.  The grid is small (~1 workgroup per CU at a 4k-token
  // step, one wave per SIMD), so memory-level parallelism has to come from the thread: on the bf16
  // path each thread issues the loads of RU items before it rotates and stores any of them ----
  __shared__ int s_slot[W], s_pos[W];
  if (threadIdx.x < W) {
    const int t = t0 + min((int)threadIdx.x, nt - 1);
    s_slot[threadIdx.x] = slot_mapping[t];
    s_pos[threadIdx.x] = positions[t];
  }
  __syncthreads();
  const int per_tok = (hq + hkv) * 8;
  const int n_items = nt * per_tok;
  auto rotate_store = [&](int j, int h, int i, const uint4& a, const uint4& b, const float4& c0, const float4& c1,
                          const float4& s0, const float4& s1) {
    const int t = t0 + j, slot = s_slot[j];
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    uint32_t o1[4], o2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xa0 = lo_f(aw[k]), xa1 = hi_f(aw[k]), xb0 = lo_f(bw[k]), xb1 = hi_f(bw[k]);
      o1[k] = pack2(xa0 * cc[2 * k] - xb0 * ss[2 * k], xa1 * cc[2 * k + 1] - xb1 * ss[2 * k + 1]);
      o2[k] = pack2(xb0 * cc[2 * k] + xa0 * ss[2 * k], xb1 * cc[2 * k + 1] + xa1 * ss[2 * k + 1]);
    }
    bf16_t* dst = h < hq ? q_out + ((size_t)t * hq + h) * d
                         : k_cache + (((size_t)(slot / bs) * hkv + (h - hq)) * bs + slot % bs) * d;
    *reinterpret_cast<uint4*>(dst + i) = make_uint4(o1[0], o1[1], o1[2], o1[3]);
    *reinterpret_cast<uint4*>(dst + i + half) = make_uint4(o2[0], o2[1], o2[2], o2[3]);
  };
  if (Pq == nullptr) {
    constexpr int RU = 4;
    for (int it0 = threadIdx.x; it0 < n_items; it0 += 256 * RU) {
      uint4 a[RU], b[RU];
      float4 c0[RU], c1[RU], s0[RU], s1[RU];
      bool ok[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int it = it0 + u * 256;
        const int j = it / per_tok, r = it - j * per_tok, h = r >> 3, i = (r & 7) * 8;
        ok[u] = it < n_items && (h < hq || s_slot[j] >= 0);
        if (ok[u]) {
          const bf16_t* row = qkv + (size_t)(t0 + j) * qkv_stride + (size_t)h * d + i;
          const float* cs = cos_sin + (size_t)s_pos[j] * d + i;
          a[u] = *reinterpret_cast<const uint4*>(row);
          b[u] = *reinterpret_cast<const uint4*>(row + half);
          c0[u] = *reinterpret_cast<const float4*>(cs);
          c1[u] = *reinterpret_cast<const float4*>(cs + 4);
          s0[u] = *reinterpret_cast<const float4*>(cs + half);
          s1[u] = *reinterpret_cast<const float4*>(cs + half + 4);
        }
      }
      asm volatile("" ::: "memory");   // all RU items' loads are issued before the first rotation
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        if (!ok[u]) continue;
        const int it = it0 + u * 256;
        const int j = it / per_tok, r = it - j * per_tok;
        rotate_store(j, r >> 3, (r & 7) * 8, a[u], b[u], c0[u], c1[u], s0[u], s1[u]);
      }
    }
  } else {   // split-K partials: ld8 sums the slices
#pragma unroll 4
    for (int it = threadIdx.x; it < n_items; it += 256) {
      const int j = it / per_tok, r = it - j * per_tok;
      const int t = t0 + j;
      const int h = r >> 3, i = (r & 7) * 8;
      if (h >= hq && s_slot[j] < 0) continue;
      const float* cs = cos_sin + (size_t)s_pos[j] * d;
      const float* prow = Pq + (size_t)t * qkv_stride;
      const uint4 a = ld8(nullptr, prow, split, pstride, (size_t)h * d + i);
      const uint4 b = ld8(nullptr, prow, split, pstride, (size_t)h * d + i + half);
      rotate_store(j, h, i, a, b, *reinterpret_cast<const float4*>(cs + i), *reinterpret_cast<const float4*>(cs + i + 4),
                   *reinterpret_cast<const float4*>(cs + half + i), *reinterpret_cast<const float4*>(cs + half + i + 4));
    }
  }
  // ---- V: per kv head, 16 tokens x 128 dims through LDS ----
  const int lj = threadIdx.x & 15;                  // store phase: lane -> token
  const int ls = slot_mapping[t0 + min(lj, nt - 1)];
  const bool lvalid = lj < nt && ls >= 0;
  const size_t vbase = (size_t)(hq + hkv) * d;
  for (int h = 0; h < hkv; ++h) {
    {   // load phase: thread -> (token, 8-dim chunk)
      const int j = threadIdx.x >> 4, c = (threadIdx.x & 15) * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (j < nt) {
        const int t = t0 + j;
        v = ld8(qkv + (size_t)t * qkv_stride, Pq ? Pq + (size_t)t * qkv_stride : nullptr, split, pstride,
                vbase + (size_t)h * d + c);
      }
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        vt[c + 2 * k][j] = (bf16_t)w[k];
        vt[c + 2 * k + 1][j] = (bf16_t)(w[k] >> 16);
      }
    }
    __syncthreads();
    if (lvalid) {
      bf16_t* dst = v_cache + ((size_t)(ls / bs) * hkv + h) * d * bs + ls % bs;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int dim = (threadIdx.x >> 4) + 16 * k;
        dst[(size_t)dim * bs] = vt[dim][lj];
      }
    }
    __syncthreads();
  }
}

static bool rope_window_ok(int tokens, int d, int bs) {
  static const int min_tok = getenv("KA_ROPE_WINDOW_MIN") ? atoi(getenv("KA_ROPE_WINDOW_MIN")) : 64;
  return tokens >= min_tok && d == 128 && bs == 16;
}

extern "C" int ka_rope_kv(void* q_out, void* k_cache, void* v_cache, const void* qkv, const int* positions,
                          const float* cos_sin, const int* slot_mapping, int tokens, int hq, int hkv, int d, int bs,
                          hipStream_t stream) {
  if (tokens <= 0) return 0;
  if (d % 16 != 0) return (int)hipErrorInvalidValue;
  if (rope_window_ok(tokens, d, bs)) {
    hipLaunchKernelGGL(rope_kv_window_kernel, dim3((tokens + 15) / 16), dim3(256), 0, stream,
                       static_cast<bf16_t*>(q_out), static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache),
                       static_cast<const bf16_t*>(qkv), positions, cos_sin, slot_mapping, tokens, hq, hkv, nullptr,
                       0, (size_t)0);
    KA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rope_kv_kernel, dim3(tokens), dim3(256), 0, stream, static_cast<bf16_t*>(q_out),
                     static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache),
                     static_cast<const bf16_t*>(qkv), positions, cos_sin, slot_mapping, hq, hkv, d, bs, nullptr, 0,
                     (size_t)0);
  KA_CHECK_LAUNCH();
}

// rope_kv over the split-K partials P [split, tokens, (hq + 2 hkv) d] of the QKV projection
extern "C" int ka_rope_kv_splitk(void* q_out, void* k_cache, void* v_cache, const void* P, int split,
                                 const int* positions, const float* cos_sin, const int* slot_mapping, int tokens,
                                 int hq, int hkv, int d, int bs, hipStream_t stream) {
  if (tokens <= 0) return 0;
  if (d % 16 != 0 || split < 1) return (int)hipErrorInvalidValue;
  const size_t pstride = (size_t)tokens * (hq + 2 * hkv) * d;
  if (rope_window_ok(tokens, d, bs)) {
    hipLaunchKernelGGL(rope_kv_window_kernel, dim3((tokens + 15) / 16), dim3(256), 0, stream,
                       static_cast<bf16_t*>(q_out), static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache),
                       nullptr, positions, cos_sin, slot_mapping, tokens, hq, hkv, static_cast<const float*>(P),
                       split, pstride);
    KA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rope_kv_kernel, dim3(tokens), dim3(256), 0, stream, static_cast<bf16_t*>(q_out),
                     static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache), nullptr, positions, cos_sin,
                     slot_mapping, hq, hkv, d, bs, static_cast<const float*>(P), split, pstride);
  KA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------
// out[t, :I] = silu(gu[t, :I]) * gu[t, I:2I]     (gate | up halves of the fused gate_up projection)
// (P != nullptr: gu is the bf16-rounded sum of `split` fp32 split-K partials of the gate_up GEMM)
__global__ __launch_bounds__(256) void silu_mul_kernel(bf16_t* __restrict__ out, const bf16_t* __restrict__ gu,
                                                       int inter, long total_vec, const float* __restrict__ P,
                                                       int split, size_t pstride) {
  const int vpr = inter >> 3;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total_vec; i += (long)gridDim.x * blockDim.x) {
    const long t = i / vpr;
    const int c = (int)(i % vpr) * 8;
    const size_t roff = (size_t)t * 2 * (size_t)inter;
    const bf16_t* r = gu ? gu + roff : nullptr;
    const float* pr = P ? P + roff : nullptr;
    uint4 g, u;
    if (pr == nullptr) {
      g = *reinterpret_cast<const uint4*>(r + c);
      u = *reinterpret_cast<const uint4*>(r + inter + c);
    } else {   // the gate and up slices in the same batches
      const size_t o[2] = {(size_t)c, (size_t)inter + c};
      f32x4 lo[2], hi[2];
      sum8_slices<2>(pr, split, pstride, o, lo, hi);
      g = make_uint4(pack2(lo[0][0], lo[0][1]), pack2(lo[0][2], lo[0][3]), pack2(hi[0][0], hi[0][1]), pack2(hi[0][2], hi[0][3]));
      u = make_uint4(pack2(lo[1][0], lo[1][1]), pack2(lo[1][2], lo[1][3]), pack2(hi[1][0], hi[1][1]), pack2(hi[1][2], hi[1][3]));
    }
    uint32_t gw[4] = {g.x, g.y, g.z, g.w}, uw[4] = {u.x, u.y, u.z, u.w}, o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float g0 = lo_f(gw[k]), g1 = hi_f(gw[k]);
      float s0 = g0 / (1.f + __expf(-g0)), s1 = g1 / (1.f + __expf(-g1));
      o[k] = pack2(s0 * lo_f(uw[k]), s1 * hi_f(uw[k]));
    }
    *reinterpret_cast<uint4*>(out + t * (long)inter + c) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

extern "C" int ka_silu_mul(void* out, const void* gu, int tokens, int inter, hipStream_t stream) {
  if (tokens <= 0) return 0;
  if (inter % 8 != 0) return (int)hipErrorInvalidValue;
  const long total = (long)tokens * (inter / 8);
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(silu_mul_kernel, dim3(grid), dim3(256), 0, stream, static_cast<bf16_t*>(out),
                     static_cast<const bf16_t*>(gu), inter, total, nullptr, 0, (size_t)0);
  KA_CHECK_LAUNCH();
}

extern "C" int ka_silu_mul_splitk(void* out, const void* P, int split, int tokens, int inter, hipStream_t stream) {
  if (tokens <= 0) return 0;
  if (inter % 8 != 0 || split < 1) return (int)hipErrorInvalidValue;
  const long total = (long)tokens * (inter / 8);
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  const size_t pstride = (size_t)tokens * 2 * inter;
  hipLaunchKernelGGL(silu_mul_kernel, dim3(grid), dim3(256), 0, stream, static_cast<bf16_t*>(out), nullptr, inter,
                     total, static_cast<const float*>(P), split, pstride);
  KA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------
// out[t, :] = table[ids[t], :]   (ids outside [0, vocab) -> zeros; vocab-parallel shards pass an offset)
__global__ __launch_bounds__(256) void embedding_kernel(bf16_t* __restrict__ out, const int* __restrict__ ids,
                                                        const bf16_t* __restrict__ table, int hidden, int vocab,
                                                        int vocab_offset) {
  const int t = blockIdx.x;
  const int id = ids[t] - vocab_offset;
  const bool valid = id >= 0 && id < vocab;
  const uint4* src = reinterpret_cast<const uint4*>(table + (size_t)(valid ? id : 0) * hidden);
  uint4* dst = reinterpret_cast<uint4*>(out + (size_t)t * hidden);
  for (int i = threadIdx.x; i < (hidden >> 3); i += blockDim.x) dst[i] = valid ? src[i] : make_uint4(0, 0, 0, 0);
}

extern "C" int ka_embedding(void* out, const int* ids, const void* table, int tokens, int hidden, int vocab,
                            int vocab_offset, hipStream_t stream) {
  if (tokens <= 0) return 0;
  if (hidden % 8 != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(embedding_kernel, dim3(tokens), dim3(256), 0, stream, static_cast<bf16_t*>(out), ids,
                     static_cast<const bf16_t*>(table), hidden, vocab, vocab_offset);
  KA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------
// Paged-KV block copy for sub-block prefix reuse (engine/block_manager.py reuse_partial): for every
// (src, dst) pair and every layer, copy the whole K block and V block (Hkv * BS * D bf16 each).
// Rows past the reused prefix are overwritten by the same step's prefill (stream order).
// grid = (pairs, layers); each block streams 2 * Hkv * BS * D * 2 bytes with 16-B accesses.
__global__ __launch_bounds__(256) void kv_block_copy_kernel(bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                            const int* __restrict__ src, const int* __restrict__ dst,
                                                            long layer_stride, long block_elems) {
  const long l = blockIdx.y;
  const long s = (long)src[blockIdx.x] * block_elems + l * layer_stride;
  const long d = (long)dst[blockIdx.x] * block_elems + l * layer_stride;
  const int nvec = (int)(block_elems / 8);
  const u32x4* ks = reinterpret_cast<const u32x4*>(kc + s);
  u32x4* kd = reinterpret_cast<u32x4*>(kc + d);
  const u32x4* vs = reinterpret_cast<const u32x4*>(vc + s);
  u32x4* vd = reinterpret_cast<u32x4*>(vc + d);
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const u32x4 a = ks[i], b = vs[i];
    kd[i] = a;
    vd[i] = b;
  }
}

extern "C" int ka_kv_block_copy(void* k_cache, void* v_cache, const void* src, const void* dst, int pairs,
                                int layers, long layer_stride, long block_elems, hipStream_t stream) {
  if (pairs <= 0) return 0;
  if (block_elems % 8 != 0 || layer_stride % 8 != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_block_copy_kernel, dim3(pairs, layers), dim3(256), 0, stream, static_cast<bf16_t*>(k_cache),
                     static_cast<bf16_t*>(v_cache), static_cast<const int*>(src), static_cast<const int*>(dst),
                     layer_stride, block_elems);
  KA_CHECK_LAUNCH();
}

// ---- weight prefetch into the Infinity Cache (MALL) ----
// Reads [p, p + bytes) once with 16-B loads and discards it (the XOR of what was read is stored only
// if it equals a value no read produces in practice, so the loads stay live): run on a side stream
// beside a kernel that leaves most CUs idle (batch-1 decode attention, RMSNorm), it turns the next
// GEMV's weight stream into MALL hits.  Read-only, no output.
__global__ __launch_bounds__(256) void prefetch_kernel(const u32x4* __restrict__ p, size_t n16, uint32_t* sink) {
  uint32_t acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
    const u32x4 v = p[i];
    acc ^= v[0] ^ v[1] ^ v[2] ^ v[3];
  }
  if (acc == 0x9e3779b9u && sink != nullptr) *sink = acc;
}

extern "C" int ka_prefetch(const void* p, long bytes, int blocks, void* sink, hipStream_t stream) {
  if (bytes <= 0) return 0;
  const size_t n16 = (size_t)bytes / 16;
  const int grid = blocks > 0 ? blocks : (int)std::min<size_t>(1024, (n16 + 255) / 256);
  hipLaunchKernelGGL(prefetch_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const u32x4*>(p), n16,
                     static_cast<uint32_t*>(sink));
  return (int)hipGetLastError();
}
