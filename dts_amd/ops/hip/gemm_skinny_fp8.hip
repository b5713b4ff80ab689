// W8A16 skinny-M MFMA GEMM for decode projections on MI355X (gfx950).
//
// out[M, N] = bf16( (x[M, K] @ deq(w_q)[N, K]^T) * scale[n] ), M = 1..16:
// FP8 (OCP e4m3fn) weights with one fp32 scale per output row, bf16
// activations, fp32 accumulation, bf16 output. The bf16 skinny GEMM
// (gemm_skinny.hip) already streams its weights at the HBM roofline, so
// the only thing left to cut is the bytes: this kernel reads half of them.
//
// The weight fragment is dequantised to bf16 IN REGISTERS
// (v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 — every finite e4m3 value is
// a bf16 value, so the conversion is exact) and feeds the same
// v_mfma_f32_16x16x32_bf16 as the bf16 kernel. Non-scaled FP8 MFMA runs at
// the bf16 rate anyway, so quantising the activations too would cost
// accuracy and buy nothing on a kernel this far from compute-bound.
//
// Structure is the bf16 kernel's: NT (1, 2 or 4) 16-row N-tiles per 4-wave
// workgroup share one A fragment, each wave owns a quarter of K, the four
// C tiles reduce through LDS. What differs is the fragment: a lane needs
// only 8 B of W per 32-k MFMA chunk, so one 16 B load covers TWO chunks —
//   B: lane (n = lane&15, g = lane>>4) loads w_q[n, k0 + g*16 + 0..15];
//      4 lanes cover one 64 B line of a W row
//   A: the same lane loads x[m = lane&15, k0 + g*16 + 0..15] (2 x 16 B)
//   elements 0..7 feed the first MFMA of the pair, 8..15 the second.
// That is a permutation of k inside each 64-k pair relative to the MFMA's
// nominal layout, which is legal because A and B use the same one: the
// MFMA only sums a[m][j] * b[n][j] over its 32 (lane group, element) slots.
// Epilogue: (red[0]+red[1]+red[2]+red[3]) * scale[n] in fp32, then ONE bf16
// rounding — or, for a fused gate_up weight, both halves rounded to bf16 and
// combined with swiglu_bf16, bit-identical to this GEMM + silu_mul.

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

#define NWAVES 4   // waves per workgroup = K split factor
#define KPAIR 64   // two mfma k-chunks = one 16 B FP8 load per lane

// 8 e4m3 bytes (two dwords) -> 8 bf16, element order = byte order
DEV bf16x8 deq8(unsigned int w0, unsigned int w1) {
  union { bf16x2 p[4]; bf16x8 v; } c;
  c.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false);
  c.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
  c.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false);
  c.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
  return c.v;
}

// KP = 64-k pairs in flight per iteration (unroll 4 -> KP 2, 8 -> KP 4, so
// the K granularity per workgroup iteration is the bf16 kernel's 512/1024).
// Tile j of workgroup b covers W rows b*wg_stride + j*tile_stride + 0..15,
// exactly as in gemm_skinny_kernel. Every output element sees the same
// arithmetic for every NT and KP (same per-wave chunk order, same
// reduction order), so results are bit-identical across them.
template <int KP, int NT, bool SWIGLU>
__global__ void __launch_bounds__(NWAVES* WAVE)
gemm_skinny_w8_kernel(short* __restrict__ out,              // [M, N]
                      const short* __restrict__ x,          // [M, K]
                      const unsigned char* __restrict__ w,  // [N, K] e4m3
                      const float* __restrict__ scale,      // [N]
                      int M, int N, int K, long x_ts, long out_ts,
                      int wg_stride, int tile_stride) {
  static_assert(!SWIGLU || NT == 2, "SwiGLU pairs one gate and one up tile");
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * wg_stride;

  // this wave's K quarter (K % (NWAVES*KPAIR*KP) checked host-side)
  const int kq = K / NWAVES;
  const int kbeg = wave * kq;
  const int kend = kbeg + kq;

  const int a_row = lane & 15;          // x row (m)
  const int k_off = (lane >> 4) * 16;   // this lane's k sub-offset in a pair
  const bool a_live = a_row < M;
  const short* xrow = x + (long)a_row * x_ts;
  // tiles past N load nothing and store nothing
  bool b_live[NT];
  const unsigned char* wrow[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int b_row = n0 + j * tile_stride + (lane & 15);  // W row (n)
    b_live[j] = b_row < N;
    wrow[j] = w + (long)(b_live[j] ? b_row : 0) * K;
  }

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const u32x4 zero4 = {0u, 0u, 0u, 0u};  // code 0x00 is +0.0

  for (int k0 = kbeg; k0 < kend; k0 += KPAIR * KP) {
    bf16x8 a[KP][2];
    u32x4 b[NT][KP];
#pragma unroll
    for (int u = 0; u < KP; ++u) {
      const int kk = k0 + u * KPAIR + k_off;
      a[u][0] = a_live ? *(const bf16x8*)(xrow + kk) : zero8;
      a[u][1] = a_live ? *(const bf16x8*)(xrow + kk + 8) : zero8;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        b[j][u] = b_live[j] ? *(const u32x4*)(wrow[j] + kk) : zero4;
    }
#pragma unroll
    for (int u = 0; u < KP; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[u][0], deq8(b[j][u][0], b[j][u][1]), acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[u][1], deq8(b[j][u][2], b[j][u][3]), acc[j], 0, 0, 0);
      }
  }

  // cross-wave reduction: C tiles are [16 m x 16 n] fp32, 1 KB per wave
  // and tile (C/D: row = (lane>>4)*4 + i, col = lane&15)
  __shared__ float red[NT][NWAVES][16][16];
  const int c_col = lane & 15;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[j][wave][(lane >> 4) * 4 + i][c_col] = acc[j][i];
  __syncthreads();
  if constexpr (SWIGLU) {
    // wave 0: gate row n scales by scale[n], its up row by scale[I + n];
    // both round to bf16 as the plain GEMM's store does, then silu_mul's
    // formula. out is [M, I], I = tile_stride.
    if (wave == 0) {
      const int n = n0 + c_col;
      if (n < tile_stride) {
        const float sg = scale[n], su = scale[tile_stride + n];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = (lane >> 4) * 4 + i;
          if (m < M) {
            float g = red[0][0][m][c_col] + red[0][1][m][c_col] +
                      red[0][2][m][c_col] + red[0][3][m][c_col];
            float u = red[1][0][m][c_col] + red[1][1][m][c_col] +
                      red[1][2][m][c_col] + red[1][3][m][c_col];
            out[(long)m * out_ts + n] = swiglu_bf16(f2bf(g * sg), f2bf(u * su));
          }
        }
      }
    }
  } else {
    // wave j writes tile j (bf16)
    for (int j = wave; j < NT; j += NWAVES) {
      const int n = n0 + j * tile_stride + c_col;
      if (n < N) {
        const float s = scale[n];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = (lane >> 4) * 4 + i;
          if (m < M) {
            float v = red[j][0][m][c_col] + red[j][1][m][c_col] +
                      red[j][2][m][c_col] + red[j][3][m][c_col];
            out[(long)m * out_ts + n] = f2bf(v * s);
          }
        }
      }
    }
  }
}

// Tiles per workgroup (NT), measured on FP8 bytes (cold weights, MI355X,
// profiles/microbench_fp8_skinny.jsonl; us at the best unroll, NT=1/2/4):
//   lm_head (8016 tiles) M=1: 93.6/94.2/97.3  M=4: 111/103/102
//                        M=8: 137/119/110     M=16: 182/142/122
//   gate_up (1792 tiles) M=4: 27.6/28.7/28.8  M=8: 32.8/31.0/30.0
//                        M=16: 42.9/36.6/32.4
//   qkv     (384 tiles)  M=8: 11.3/11.5/15.3  M=16: 13.8/12.0/16.2
//   o / down (256 tiles) NT=1 everywhere (NT=2 is +10-25%)
// Sharing the A fragment pays EARLIER than on bf16 weights (lm_head from
// M=4, gate_up from M=8 where bf16 is flat): the weight bytes per tile
// halved while the activation bytes did not. Keyed on M and the tile count
// and measured ONLY at M = 1, 4, 8, 16 on these five Llama-3-8B shapes; M
// in between and other (K, N) fall into the same bands unmeasured.
static int w8_auto_tiles(int M, int tiles) {
  if (tiles >= 4096) return M >= 4 ? 4 : 1;
  if (tiles >= 1024) return M >= 8 ? 4 : 1;
  if (tiles >= 384) return M > 8 ? 2 : 1;
  return 1;
}

// k-chunks in flight per iteration, in the bf16 kernel's unit (32-k MFMA
// chunks): 4 = two 64-k pairs, 8 = four. Measured (same file): a lane has
// half the bytes in flight per chunk of an FP8 weight, and at ONE tile per
// workgroup the deeper unroll wins on every shape, not only the deep-K
// one as for bf16 (M=1/4/8, us at 4 -> 8: o 9.2/9.7/9.9 -> 8.0/8.4/8.9,
// qkv 9.7/10.4/11.3 -> 8.6/9.9/11.3, down 25.0/25.7/25.7 ->
// 19.5/20.0/20.8, gate_up and lm_head -1 us). With 2 tiles the loads of
// the second tile already give that depth: 8 only helps deep K (down at
// NT=2 29.0 -> 23.0) and is flat elsewhere; with 4 tiles 8 is flat to
// worse everywhere (down M=8 39.9 -> 44.3).
static int w8_unroll(int K, int nt, int64_t unroll) {
  TORCH_CHECK(unroll != 8 || K % (NWAVES * KPAIR * 4) == 0,
              "unroll=8 needs K % 1024 == 0, got K=", K);
  if (unroll) return (int)unroll;
  if (K % (NWAVES * KPAIR * 4) != 0) return 4;
  return (nt == 1 || (nt == 2 && K >= 8192)) ? 8 : 4;
}

static void w8_check(const torch::Tensor& out, const torch::Tensor& x,
                     const torch::Tensor& w_q, const torch::Tensor& scale) {
  TORCH_CHECK(x.is_cuda() && w_q.is_cuda() && scale.is_cuda() && out.is_cuda(),
              "all operands must be device tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && w_q.dim() == 2);
  TORCH_CHECK(w_q.element_size() == 1, "w_q must be 1 byte per element");
  TORCH_CHECK(w_q.is_contiguous(), "w_q must be contiguous [N, K]");
  TORCH_CHECK(x.stride(1) == 1, "x rows must be dense");
  TORCH_CHECK(out.stride(1) == 1);
  const int64_t M = x.size(0), K = x.size(1), N = w_q.size(0);
  TORCH_CHECK(M >= 1 && M <= 16, "skinny path is for M<=16");
  TORCH_CHECK(K % (NWAVES * KPAIR * 2) == 0, "K must be /512");
  TORCH_CHECK(w_q.size(1) == K && out.size(0) == M);
  TORCH_CHECK(scale.scalar_type() == torch::kFloat32 && scale.dim() == 1 &&
                  scale.size(0) == N && scale.is_contiguous(),
              "scale must be contiguous fp32 [N]");
}

#define W8_LAUNCH(KP_, NT_, SW_, grid_, wgs_, ts_)                            \
  hipLaunchKernelGGL((gemm_skinny_w8_kernel<KP_, NT_, SW_>), dim3(grid_),    \
                     dim3(NWAVES * WAVE), 0, stream, (short*)out.data_ptr(), \
                     (const short*)x.data_ptr(),                             \
                     (const unsigned char*)w_q.data_ptr(),                   \
                     (const float*)scale.data_ptr(), M, N, K, x.stride(0),   \
                     out.stride(0), wgs_, ts_)

void gemm_skinny_w8_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w_q,
                         torch::Tensor scale, int64_t tiles_per_wg,
                         int64_t unroll) {
  w8_check(out, x, w_q, scale);
  const int M = x.size(0), K = x.size(1), N = w_q.size(0);
  TORCH_CHECK(out.size(1) == N);
  TORCH_CHECK(tiles_per_wg == 0 || tiles_per_wg == 1 || tiles_per_wg == 2 ||
                  tiles_per_wg == 4,
              "tiles_per_wg must be 0 (auto), 1, 2 or 4");
  TORCH_CHECK(unroll == 0 || unroll == 4 || unroll == 8,
              "unroll must be 0 (auto), 4 or 8");
  const int tiles = (N + 15) / 16;
  const int nt = tiles_per_wg ? (int)tiles_per_wg : w8_auto_tiles(M, tiles);
  const int grid = (tiles + nt - 1) / nt;
  auto stream = c10::hip::getCurrentHIPStream();
  if (w8_unroll(K, nt, unroll) == 8) {
    if (nt == 4) W8_LAUNCH(4, 4, false, grid, 64, 16);
    else if (nt == 2) W8_LAUNCH(4, 2, false, grid, 32, 16);
    else W8_LAUNCH(4, 1, false, grid, 16, 16);
  } else {
    if (nt == 4) W8_LAUNCH(2, 4, false, grid, 64, 16);
    else if (nt == 2) W8_LAUNCH(2, 2, false, grid, 32, 16);
    else W8_LAUNCH(2, 1, false, grid, 16, 16);
  }
  HIP_CHECK_LAST();
}

// out[M, I] = silu(gate) * up with gate = bf16((x Wg^T) * scale[:I]) and
// up = bf16((x Wu^T) * scale[I:]), w_q = [Wg ; Wu] of shape [2I, K].
void gemm_skinny_swiglu_w8_bf16(torch::Tensor out, torch::Tensor x,
                                torch::Tensor w_q, torch::Tensor scale) {
  w8_check(out, x, w_q, scale);
  const int M = x.size(0), K = x.size(1), N = w_q.size(0);
  const int I = N / 2;
  TORCH_CHECK(N == 2 * I && I % 16 == 0, "fused SwiGLU needs I % 16 == 0");
  TORCH_CHECK(out.size(1) == I);
  const int grid = I / 16;
  auto stream = c10::hip::getCurrentHIPStream();
  if (w8_unroll(K, 2, 0) == 8)
    W8_LAUNCH(4, 2, true, grid, 16, I);
  else
    W8_LAUNCH(2, 2, true, grid, 16, I);
  HIP_CHECK_LAST();
}
#undef W8_LAUNCH
