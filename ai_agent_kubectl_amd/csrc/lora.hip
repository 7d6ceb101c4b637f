// Per-request LoRA adapters: y += scale * (x A^T) B^T with the adapter chosen per row (`row_adapter`, -1 = none).
// Semantics: ops/reference.py `lora_add`.  x bf16 [T, K], y bf16 [T, N], A bf16 [n_adapters, S, R, K],
// B bf16 [n_adapters, N, R], scale fp32 [n_adapters, S]; the S segments of N (q | k | v, gate | up) each have
// their own A block and scale; R = 16, 32 or 64 is the padded rank.
//
// Two kernels, both on v_mfma_f32_16x16x32_bf16, operands loaded straight from global memory (16 B per lane; the
// adapter matrices are small and stay in L2), no atomics:
//
//  * shrink: grid (16-row tile, segment, K split).  The four waves of a workgroup and the `splits` workgroups share
//    the K / 32 k-steps in contiguous chunks.  Per adapter present in the tile (a wave-uniform loop over the adapter
//    slots) the wave accumulates the 16 x R tile x A^T, the four waves are summed through LDS in wave order, and the
//    rows that carry this adapter write their fp32 partial to ws [splits, T, S, R].  Every (row, segment) with a
//    live adapter and a nonzero scale is written by every split, so the expand kernel never reads a stale word.
//  * expand: grid (16-row tile, LORA_TN columns).  A wave takes 16-column blocks; a block lies in one segment since
//    the boundaries are multiples of 16.  t = bf16(sum of the partials in split order): the rounding is part of the
//    definition.  The product is taken transposed, D^T = B t^T, so that a lane holds four consecutive columns of one
//    row of y: 8-byte loads and stores.  A lane of a row with another adapter computes on that row's own t and
//    drops the result (the columns of D^T are independent), so t is loaded once per segment, not per adapter.
//
// Rows >= T, rows of -1 (or an index outside [0, n_adapters)) and segments of scale 0 are neither read nor written.
#include "common.h"

namespace {

constexpr int LORA_ROWS = 16;          // rows per tile: the MFMA's M
constexpr int LORA_NT = 256;           // threads per workgroup
constexpr int LORA_WAVES = LORA_NT / 64;
constexpr int LORA_TN = 256;           // expand: columns per workgroup (LORA_WAVES x LORA_NB 16-column blocks)
constexpr int LORA_NB = LORA_TN / (16 * LORA_WAVES);
constexpr int LORA_MAX_SEG = 4;
constexpr int LORA_MAX_ADAPTERS = 8;
constexpr int LORA_MAX_SPLITS = 16;

struct LoraSeg {
  int b[LORA_MAX_SEG + 1];
};

// bit a set: some row of the tile carries adapter a (wave-uniform; every wave computes the same word)
KA_DEV uint32_t lora_present(const int* __restrict__ row_adapter, int row0, int T, int n_adapters, int lane, int& mine) {
  const int r = row0 + (lane & 15);
  int a = r < T ? row_adapter[r] : -1;
  if (a < 0 || a >= n_adapters) a = -1;
  mine = a;
  uint32_t m = 0u;
  for (int i = 0; i < n_adapters; ++i)
    if (__ballot(a == i) != 0ull) m |= 1u << i;
  return m;
}

template <int RB>   // R = 16 RB
__global__ __launch_bounds__(LORA_NT) void lora_shrink_kernel(float* __restrict__ ws, const bf16_t* __restrict__ x,
                                                              const int* __restrict__ row_adapter,
                                                              const bf16_t* __restrict__ A,
                                                              const float* __restrict__ scale, int T, int K, int S,
                                                              int n_adapters, int splits) {
  constexpr int R = 16 * RB;
  __shared__ float s_acc[LORA_WAVES][LORA_ROWS][R];
  __shared__ int s_adp[LORA_ROWS];
  const int row0 = blockIdx.x * LORA_ROWS, s = blockIdx.y, ks = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  int mine;
  const uint32_t present = lora_present(row_adapter, row0, T, n_adapters, lane, mine);
  if (threadIdx.x < LORA_ROWS) s_adp[threadIdx.x] = mine;
  // this wave's k-steps
  const int nk = K >> 5, nw = splits * LORA_WAVES, w = ks * LORA_WAVES + wave;
  const int k_lo = (int)((long)nk * w / nw), k_hi = (int)((long)nk * (w + 1) / nw);
  const bool row_ok = row0 + col < T;
  const bf16_t* xr = x + (size_t)(row_ok ? row0 + col : 0) * K + 8 * grp;
  for (int a = 0; a < n_adapters; ++a) {
    if (!((present >> a) & 1u) || scale[a * S + s] == 0.f) continue;   // uniform over the workgroup
    const bf16_t* ar = A + ((size_t)(a * S + s) * R + col) * K + 8 * grp;
    f32x4 acc[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = k_lo; k < k_hi; ++k) {
      uint4 xv = make_uint4(0u, 0u, 0u, 0u);
      if (row_ok) xv = *reinterpret_cast<const uint4*>(xr + (size_t)k * 32);
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const uint4 av = *reinterpret_cast<const uint4*>(ar + (size_t)j * 16 * K + (size_t)k * 32);
        acc[j] = mfma16x16x32(as_bf16x8(xv), as_bf16x8(av), acc[j]);   // C: column = rank index, rows 4 grp + r
      }
    }
    __syncthreads();   // the previous adapter's sums have been read
#pragma unroll
    for (int j = 0; j < RB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) s_acc[wave][4 * grp + r][16 * j + col] = acc[j][r];
    __syncthreads();
    for (int e = threadIdx.x; e < LORA_ROWS * R; e += LORA_NT) {
      const int r = e / R, j = e % R;
      if (s_adp[r] != a) continue;   // implies row0 + r < T
      float v = s_acc[0][r][j];
#pragma unroll
      for (int q = 1; q < LORA_WAVES; ++q) v += s_acc[q][r][j];
      ws[(((size_t)ks * T + row0 + r) * S + s) * R + j] = v;
    }
  }
}

template <int RB>
__global__ __launch_bounds__(LORA_NT) void lora_expand_kernel(bf16_t* __restrict__ y, const float* __restrict__ ws,
                                                              const int* __restrict__ row_adapter,
                                                              const bf16_t* __restrict__ B,
                                                              const float* __restrict__ scale, LoraSeg seg, int T,
                                                              int N, int S, int n_adapters, int splits) {
  constexpr int R = 16 * RB;
  constexpr int KK = (R + 31) / 32;   // MFMA k-steps over the rank; R = 16 fills half of one
  const int row0 = blockIdx.x * LORA_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  int mine;
  const uint32_t present = lora_present(row_adapter, row0, T, n_adapters, lane, mine);
  const int row = row0 + col;
  int cur_s = -1;
  uint4 tf[KK];
  for (int b = 0; b < LORA_NB; ++b) {
    const int n0 = blockIdx.y * LORA_TN + (wave * LORA_NB + b) * 16;
    if (n0 >= N) break;   // uniform over the wave
    int s = 0;
    while (s + 1 < S && n0 >= seg.b[s + 1]) ++s;
    if (s != cur_s) {   // t of this lane's row under the row's own adapter, rank indices 32 kk + 8 grp ..
      cur_s = s;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int j0 = 32 * kk + 8 * grp;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (mine >= 0 && j0 < R && scale[mine * S + s] != 0.f) {
          for (int q = 0; q < splits; ++q) {   // fixed order
            const float4* p = reinterpret_cast<const float4*>(ws + (((size_t)q * T + row) * S + s) * R + j0);
            const float4 lo = p[0], hi = p[1];
            v[0] += lo.x; v[1] += lo.y; v[2] += lo.z; v[3] += lo.w;
            v[4] += hi.x; v[5] += hi.y; v[6] += hi.z; v[7] += hi.w;
          }
        }
        tf[kk] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
      }
    }
    for (int a = 0; a < n_adapters; ++a) {
      if (!((present >> a) & 1u)) continue;   // uniform
      const float sc = scale[a * S + s];
      if (sc == 0.f) continue;                // uniform
      const bf16_t* br = B + ((size_t)a * N + n0 + col) * R + 8 * grp;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        uint4 bv = make_uint4(0u, 0u, 0u, 0u);
        if (32 * kk + 8 * grp < R) bv = *reinterpret_cast<const uint4*>(br + 32 * kk);
        acc = mfma16x16x32(as_bf16x8(bv), as_bf16x8(tf[kk]), acc);   // C: column = token row, rows = n0 + 4 grp + r
      }
      if (mine == a) {   // implies row < T
        uint2* yp = reinterpret_cast<uint2*>(y + (size_t)row * N + n0 + 4 * grp);
        const uint2 o = *yp;
        uint2 w;
        w.x = pack2(__fadd_rn(lo_f(o.x), __fmul_rn(sc, acc[0])), __fadd_rn(hi_f(o.x), __fmul_rn(sc, acc[1])));
        w.y = pack2(__fadd_rn(lo_f(o.y), __fmul_rn(sc, acc[2])), __fadd_rn(hi_f(o.y), __fmul_rn(sc, acc[3])));
        *yp = w;
      }
    }
  }
}

int lora_splits(int T, int S, int K) {
  if (T <= 0 || S <= 0 || K < 32) return 1;
  const int tiles = (T + LORA_ROWS - 1) / LORA_ROWS;
  const int by_k = (K >> 5) / (LORA_WAVES * 8);            // at least 8 k-steps per wave
  const int by_grid = 1024 / (tiles * S);                  // about four workgroups per CU at the most
  int n = by_k < by_grid ? by_k : by_grid;
  if (n > LORA_MAX_SPLITS) n = LORA_MAX_SPLITS;
  return n < 1 ? 1 : n;
}

}  // namespace

// the geometry the tests straddle: rows per tile, columns per expand workgroup, K splits of a shape
extern "C" int ka_lora_tile_rows() { return LORA_ROWS; }
extern "C" int ka_lora_tile_n() { return LORA_TN; }
extern "C" int ka_lora_splits(int T, int S, int K) { return lora_splits(T, S, K); }

// y [T, N] += scale * (x [T, K] A^T) B^T per row_adapter.  seg: HOST int [S + 1] (0 = seg[0] < ... < seg[S] = N,
// multiples of 16); ws: device fp32 [ka_lora_splits(T, S, K), T, S, R].
extern "C" int ka_lora_add(void* y, const void* x, const int* row_adapter, const void* A, const void* B,
                           const float* scale, const int* seg, void* ws, int T, int N, int K, int S, int R,
                           int n_adapters, hipStream_t stream) {
  if (y == nullptr || x == nullptr || row_adapter == nullptr || A == nullptr || B == nullptr || scale == nullptr ||
      seg == nullptr || ws == nullptr)
    return (int)hipErrorInvalidValue;
  if (T < 0 || N <= 0 || K <= 0 || K % 64 != 0 || N % 16 != 0 || S < 1 || S > LORA_MAX_SEG ||
      (R != 16 && R != 32 && R != 64) || n_adapters < 1 || n_adapters > LORA_MAX_ADAPTERS)
    return (int)hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(A) |
        reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(ws)) & 15u) != 0)
    return (int)hipErrorInvalidValue;
  LoraSeg sg;
  for (int i = 0; i <= LORA_MAX_SEG; ++i) sg.b[i] = N;
  if (seg[0] != 0 || seg[S] != N) return (int)hipErrorInvalidValue;
  for (int i = 0; i <= S; ++i) {
    if (seg[i] % 16 != 0 || (i > 0 && seg[i] <= seg[i - 1])) return (int)hipErrorInvalidValue;
    sg.b[i] = seg[i];
  }
  if (T == 0) return 0;
  const int tiles = (T + LORA_ROWS - 1) / LORA_ROWS;
  if (tiles > 65535 * 16) return (int)hipErrorInvalidValue;
  const int splits = lora_splits(T, S, K);
  const dim3 gs(tiles, S, splits), ge(tiles, (N + LORA_TN - 1) / LORA_TN);
  float* w = static_cast<float*>(ws);
  const bf16_t* xp = static_cast<const bf16_t*>(x);
  const bf16_t* Ap = static_cast<const bf16_t*>(A);
  const bf16_t* Bp = static_cast<const bf16_t*>(B);
  bf16_t* yp = static_cast<bf16_t*>(y);
#define KA_LORA_LAUNCH(RB)                                                                                          \
  hipLaunchKernelGGL(lora_shrink_kernel<RB>, gs, dim3(LORA_NT), 0, stream, w, xp, row_adapter, Ap, scale, T, K, S,  \
                     n_adapters, splits);                                                                           \
  hipLaunchKernelGGL(lora_expand_kernel<RB>, ge, dim3(LORA_NT), 0, stream, yp, w, row_adapter, Bp, scale, sg, T, N, \
                     S, n_adapters, splits)
  if (R == 16) {
    KA_LORA_LAUNCH(1);
  } else if (R == 32) {
    KA_LORA_LAUNCH(2);
  } else {
    KA_LORA_LAUNCH(4);
  }
#undef KA_LORA_LAUNCH
  KA_CHECK_LAUNCH();
}
