// W4A16 skinny-M MFMA GEMM for decode projections on MI355X (gfx950).
//
// out[M, N] = bf16( x[M, K] @ deq(w_q, scale)[N, K]^T ), M = 1..16:
// OCP MXFP4 weights — e2m1 codes, two per byte (element 2i in the low
// nibble of byte i, 2i+1 in the high nibble), in blocks of 32 along K with
// one e8m0 scale byte per block (value 2^(b-127)) — bf16 activations, fp32
// accumulation, bf16 output. A quarter of the bf16 kernel's weight bytes.
//
// The weight fragment is dequantised to bf16 IN REGISTERS by
// v_cvt_scalef32_pk_bf16_fp4: one byte (two codes) and a power-of-two scale
// operand in, a bf16 pair out. An e2m1 value has two significant bits and
// the scale is a power of two, so code * scale is exactly a bf16 value and
// the MFMA (v_mfma_f32_16x16x32_bf16, as in the bf16 and W8 kernels) sees
// the dequantised matrix itself. The block scale rides on the conversion,
// so there is no epilogue multiply: one f2bf of the reduced sum.
//
// Structure is the bf16 / W8 kernels': NT (1, 2 or 4) 16-row N-tiles per
// 4-wave workgroup share one A fragment, each wave owns a quarter of K, the
// four C tiles reduce through LDS as red0+red1+red2+red3, wave j stores
// tile j, ragged or dead tiles load and store nothing, and tile j of
// workgroup b covers W rows b*wg_stride + j*tile_stride + 0..15 (the fused
// SwiGLU twin is NT = 2 with tile stride I).
//
// The fragment is new. The unit is a 128-k QUAD = 4 MFMAs:
//   B: lane (n = lane&15, g = lane>>4) issues one 16 B load,
//      w_q[n, (k0 + 32g)/2 .. +16): 32 codes = exactly ONE MX block, so the
//      lane needs one scale byte, scale[n, k0/32 + g], for all 16
//      conversions of that load. The 4 lanes of a row cover one 64 B line.
//      Dword j of the load (codes 8j..8j+7) feeds MFMA j of the quad.
//   A: the same lane loads x[m = lane&15, k0 + 32g + 8j .. +8) for MFMA
//      j = 0..3 (4 x 16 B, one 64 B line per lane).
// So a wave keeps 16 B of weights and 64 B of activations per lane in
// flight per quad, where the W8 kernel's 64-k pair has 16 B and 32 B.
// MFMA j of a quad therefore sums k0 + 32g + 8j + e over (g, e) where the
// nominal layout sums k0 + 32j + 8g + e: a permutation of k inside each
// 128-k quad. It is legal because A and B use the same one — the MFMA only
// sums a[m][s] * b[n][s] over its 32 (lane group, element) slots.
//   Scales: k0 is a multiple of 128, so the four scale bytes of a quad are
//      one aligned dword scale[n, k0/32 .. +4); every lane of the row loads
//      it (one broadcast request) and takes byte g. (byte << 23) is the
//      fp32 2^(b-127), the conversion's scale operand.
//
// The instruction takes the LOW nibble of the selected byte as element 0 of
// the pair and the high nibble as element 1, which is the storage order.

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

#define NWAVES 4    // waves per workgroup = K split factor
#define KQUAD 128   // four mfma k-chunks = one 16 B MXFP4 load per lane

// 4 bytes = 8 e2m1 codes -> 8 bf16 (code * s), element order = nibble order
DEV bf16x8 deq8_fp4(unsigned int w, float s) {
  union { bf16x2 p[4]; bf16x8 v; } c;
  c.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0);
  c.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1);
  c.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2);
  c.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3);
  return c.v;
}

// KQ = 128-k quads in flight per iteration (unroll 4 -> 1, 8 -> 2, 16 -> 4,
// so unroll keeps the bf16 kernel's unit of 32-k chunks). Every output
// element sees the same arithmetic for every NT and KQ (same per-wave quad
// order, same reduction order), so results are bit-identical across them.
template <int KQ, int NT, bool SWIGLU>
__global__ void __launch_bounds__(NWAVES* WAVE)
gemm_skinny_w4_kernel(short* __restrict__ out,                  // [M, N]
                      const short* __restrict__ x,              // [M, K]
                      const unsigned char* __restrict__ w,      // [N, K/2]
                      const unsigned char* __restrict__ scale,  // [N, K/32]
                      int M, int N, int K, long x_ts, long out_ts,
                      int wg_stride, int tile_stride) {
  static_assert(!SWIGLU || NT == 2, "SwiGLU pairs one gate and one up tile");
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * wg_stride;

  // this wave's K quarter (K % (NWAVES*KQUAD*KQ) checked host-side)
  const int kq = K / NWAVES;
  const int kbeg = wave * kq;
  const int kend = kbeg + kq;

  const int a_row = lane & 15;     // x row (m)
  const int g = lane >> 4;         // MX block of the quad this lane owns
  const int k_off = g * 32;        // its k sub-offset in the quad
  const bool a_live = a_row < M;
  const short* xrow = x + (long)a_row * x_ts;
  // tiles past N load nothing and store nothing
  bool b_live[NT];
  const unsigned char* wrow[NT];
  const unsigned char* srow[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int b_row = n0 + j * tile_stride + (lane & 15);  // W row (n)
    b_live[j] = b_row < N;
    wrow[j] = w + (long)(b_live[j] ? b_row : 0) * (K / 2);
    srow[j] = scale + (long)(b_live[j] ? b_row : 0) * (K / 32);
  }

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const u32x4 zero4 = {0u, 0u, 0u, 0u};  // code 0x0 is +0.0
  const unsigned int one4 = 0x7f7f7f7fu;  // scale bytes of a dead tile: 2^0

  for (int k0 = kbeg; k0 < kend; k0 += KQUAD * KQ) {
    bf16x8 a[KQ][4];
    u32x4 b[NT][KQ];
    unsigned int sc[NT][KQ];
#pragma unroll
    for (int u = 0; u < KQ; ++u) {
      const int kk = k0 + u * KQUAD;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        b[j][u] = b_live[j] ? *(const u32x4*)(wrow[j] + (kk + k_off) / 2) : zero4;
        sc[j][u] = b_live[j] ? *(const unsigned int*)(srow[j] + kk / 32) : one4;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[u][i] = a_live ? *(const bf16x8*)(xrow + kk + k_off + 8 * i) : zero8;
    }
#pragma unroll
    for (int u = 0; u < KQ; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        // this lane's block scale: byte g of the quad's dword, as 2^(b-127)
        const float s = __uint_as_float(((sc[j][u] >> (8 * g)) & 0xffu) << 23);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[u][i], deq8_fp4(b[j][u][i], s), acc[j], 0, 0, 0);
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
    // wave 0: gate tile 0, up tile 1, both rounded to bf16 as the plain
    // GEMM's store does, then silu_mul's formula. out is [M, I],
    // I = tile_stride.
    if (wave == 0) {
      const int n = n0 + c_col;
      if (n < tile_stride) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = (lane >> 4) * 4 + i;
          if (m < M) {
            float gt = red[0][0][m][c_col] + red[0][1][m][c_col] +
                       red[0][2][m][c_col] + red[0][3][m][c_col];
            float up = red[1][0][m][c_col] + red[1][1][m][c_col] +
                       red[1][2][m][c_col] + red[1][3][m][c_col];
            out[(long)m * out_ts + n] = swiglu_bf16(f2bf(gt), f2bf(up));
          }
        }
      }
    }
  } else {
    // wave j writes tile j (bf16)
    for (int j = wave; j < NT; j += NWAVES) {
      const int n = n0 + j * tile_stride + c_col;
      if (n < N) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = (lane >> 4) * 4 + i;
          if (m < M) {
            float v = red[j][0][m][c_col] + red[j][1][m][c_col] +
                      red[j][2][m][c_col] + red[j][3][m][c_col];
            out[(long)m * out_ts + n] = f2bf(v);
          }
        }
      }
    }
  }
}

// Tiles per workgroup (NT), measured on MXFP4 bytes (cold weights, MI355X,
// profiles/microbench_fp4_skinny.jsonl; us at the best unroll, NT=1/2/4):
//   lm_head (8016 tiles) M=1: 87.9/75.6/76.6  M=4: 108/87.0/81.5
//                        M=8: 132/100/88.3    M=16: 192/133/102
//   gate_up (1792 tiles) M=1: 22.5/22.3/21.5  M=4: 26.6/24.9/23.2
//                        M=8: 32.2/27.6/24.9  M=16: 44.8/35.1/28.5
//   qkv     (384 tiles)  M=4: 9.5/9.6/14.2    M=8: 10.8/10.3/14.9
//                        M=16: 13.8/11.1/15.0
//   o / down (256 tiles) NT=1 everywhere (NT=2 is +15-45%)
// Sharing the A fragment pays earlier again than on FP8 weights (gate_up
// and lm_head at every M): a tile's weight bytes halved once more while the
// 64 B of activations per lane per quad did not. Keyed on M and the tile
// count and measured ONLY at M = 1, 4, 8, 16 on these five Llama-3-8B
// shapes; M in between and other (K, N) fall into the same bands unmeasured.
static int w4_auto_tiles(int M, int tiles) {
  if (tiles >= 4096) return M >= 4 ? 4 : 2;
  if (tiles >= 1024) return 4;
  if (tiles >= 384) return M >= 8 ? 2 : 1;
  return 1;
}

// k-chunks in flight per iteration, in the bf16 kernel's unit (32-k MFMA
// chunks): 4 = one 128-k quad, 8 = two, 16 = four. An explicit unroll on a
// K it does not divide is an error; auto takes the deepest unroll that
// divides K and does not exceed the one these rules want. Measured (same
// file, us at unroll 4/8/16):
//   NT=1, 256 tiles: o M=1 7.6/7.5/6.2, M=4 8.2/8.3/7.2, M=8 8.2/8.7/7.8,
//     M=16 8.8/9.3/9.4; down (K=14336) M=1 24.5/20.9/17.0, M=4
//     22.9/22.0/19.2, M=8 22.1/20.8/21.7, M=16 23.6/22.9/25.0. Four quads
//     in flight at narrow M (one 16 B weight load per quad is little to
//     cover latency with); at wide M the 64 B of activations per quad take
//     over and the depth costs registers: back to 8 on deep K, 4 otherwise.
//   NT=1, qkv (384 tiles): M=1 8.8/8.3/8.9, M=4 9.8/9.5/10.3 -> 8.
//   NT=2: qkv M=8 10.6/10.9/10.3, M=16 11.1/11.8/12.0; lm_head M=1
//     78.8/77.9/75.6 -> 16 up to M=8, 4 above.
//   NT=4: gate_up 4 at every M (M=1 21.5/23.6/22.9, M=16 28.5/28.9/29.6);
//     lm_head 8 (M=4 84.2/81.5/84.1, M=8 91.3/88.3/90.0, M=16
//     107.8/104.1/102.1).
static int w4_unroll(int M, int K, int tiles, int nt, int64_t unroll) {
  TORCH_CHECK(unroll != 8 || K % (NWAVES * KQUAD * 2) == 0,
              "unroll=8 needs K % 1024 == 0, got K=", K);
  TORCH_CHECK(unroll != 16 || K % (NWAVES * KQUAD * 4) == 0,
              "unroll=16 needs K % 2048 == 0, got K=", K);
  if (unroll) return (int)unroll;
  int want;
  if (nt == 1 && tiles < 384)
    want = M <= 4 ? 16 : (K >= 8192 ? 8 : (M <= 8 ? 16 : 4));
  else if (nt == 1)
    want = 8;
  else if (nt == 2)
    want = M <= 8 ? 16 : 4;
  else
    want = tiles >= 4096 ? 8 : 4;
  while (K % (NWAVES * 32 * want) != 0) want /= 2;  // K % 512 == 0 ends it
  return want;
}

static void w4_check(const torch::Tensor& out, const torch::Tensor& x,
                     const torch::Tensor& w_q, const torch::Tensor& scale) {
  TORCH_CHECK(x.is_cuda() && w_q.is_cuda() && scale.is_cuda() && out.is_cuda(),
              "all operands must be device tensors");
  TORCH_CHECK(x.get_device() == out.get_device() &&
                  x.get_device() == w_q.get_device() &&
                  x.get_device() == scale.get_device(),
              "all operands must be on the same device");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
                  out.scalar_type() == torch::kBFloat16,
              "x and out must be bf16");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && w_q.dim() == 2);
  TORCH_CHECK(w_q.scalar_type() == torch::kUInt8, "w_q must be uint8");
  TORCH_CHECK(w_q.is_contiguous(), "w_q must be contiguous [N, K/2]");
  TORCH_CHECK(x.stride(1) == 1, "x rows must be dense");
  TORCH_CHECK(out.stride(1) == 1, "out rows must be dense");
  const int64_t M = x.size(0), K = x.size(1), N = w_q.size(0);
  TORCH_CHECK(M >= 1 && M <= 16, "skinny path is for M<=16");
  TORCH_CHECK(K % (NWAVES * KQUAD) == 0, "K must be /512");
  // the kernel reads x and w_q rows as 16 B vectors
  TORCH_CHECK(x.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "x rows must be 16 B aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w_q.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(scale.data_ptr()) % 4 == 0,
              "w_q must be 16 B aligned and scale 4 B aligned");
  TORCH_CHECK(w_q.size(1) * 2 == K, "w_q must be [N, K/2], two codes a byte");
  TORCH_CHECK(out.size(0) == M);
  TORCH_CHECK(scale.scalar_type() == torch::kUInt8 && scale.dim() == 2 &&
                  scale.size(0) == N && scale.size(1) * 32 == K &&
                  scale.is_contiguous(),
              "scale must be contiguous uint8 (e8m0) [N, K/32]");
}

#define W4_LAUNCH(KQ_, NT_, SW_, grid_, wgs_, ts_)                            \
  hipLaunchKernelGGL((gemm_skinny_w4_kernel<KQ_, NT_, SW_>), dim3(grid_),    \
                     dim3(NWAVES * WAVE), 0, stream, (short*)out.data_ptr(), \
                     (const short*)x.data_ptr(),                             \
                     (const unsigned char*)w_q.data_ptr(),                   \
                     (const unsigned char*)scale.data_ptr(), M, N, K,        \
                     x.stride(0), out.stride(0), wgs_, ts_)

#define W4_LAUNCH_NT(KQ_)                                  \
  do {                                                     \
    if (nt == 4) W4_LAUNCH(KQ_, 4, false, grid, 64, 16);   \
    else if (nt == 2) W4_LAUNCH(KQ_, 2, false, grid, 32, 16); \
    else W4_LAUNCH(KQ_, 1, false, grid, 16, 16);           \
  } while (0)

void gemm_skinny_w4_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w_q,
                         torch::Tensor scale, int64_t tiles_per_wg,
                         int64_t unroll) {
  w4_check(out, x, w_q, scale);
  const int M = x.size(0), K = x.size(1), N = w_q.size(0);
  TORCH_CHECK(out.size(1) == N);
  TORCH_CHECK(tiles_per_wg == 0 || tiles_per_wg == 1 || tiles_per_wg == 2 ||
                  tiles_per_wg == 4,
              "tiles_per_wg must be 0 (auto), 1, 2 or 4");
  TORCH_CHECK(unroll == 0 || unroll == 4 || unroll == 8 || unroll == 16,
              "unroll must be 0 (auto), 4, 8 or 16");
  const int tiles = (N + 15) / 16;
  const int nt = tiles_per_wg ? (int)tiles_per_wg : w4_auto_tiles(M, tiles);
  const int grid = (tiles + nt - 1) / nt;
  auto stream = c10::hip::getCurrentHIPStream();
  const int ku = w4_unroll(M, K, tiles, nt, unroll);
  if (ku == 16) W4_LAUNCH_NT(4);
  else if (ku == 8) W4_LAUNCH_NT(2);
  else W4_LAUNCH_NT(1);
  HIP_CHECK_LAST();
}

// out[M, I] = silu(gate) * up with gate = bf16(x Wg^T) and up = bf16(x Wu^T),
// w_q = [Wg ; Wu] of shape [2I, K/2], scale [2I, K/32].
void gemm_skinny_swiglu_w4_bf16(torch::Tensor out, torch::Tensor x,
                                torch::Tensor w_q, torch::Tensor scale) {
  w4_check(out, x, w_q, scale);
  const int M = x.size(0), K = x.size(1), N = w_q.size(0);
  const int I = N / 2;
  TORCH_CHECK(N == 2 * I, "fused SwiGLU needs an even row count [Wg ; Wu]");
  TORCH_CHECK(out.size(1) == I);
  // I need not be whole tiles: the last workgroup's gate tile runs into the
  // up rows, which it multiplies but does not store (n < tile_stride)
  const int grid = (I + 15) / 16;
  auto stream = c10::hip::getCurrentHIPStream();
  // one quad in flight: the depth this kernel was measured at (the plain
  // GEMM at NT=2 is flat in unroll on the gate_up shape, 23.0/22.3/22.4)
  W4_LAUNCH(1, 2, true, grid, 16, I);
  HIP_CHECK_LAST();
}
#undef W4_LAUNCH_NT
#undef W4_LAUNCH
