// Skinny-M MFMA GEMM for decode projections on MI355X (gfx950).
//
// out[M, N] = x[M, K] @ W[N, K]^T with M = decode batch width (3..16).
// The round-1 VALU GEMV (gemv.hip) hits the HBM roofline at M<=2 but
// turns ALU-bound past M≈8 (RPW*M*8 scalar FMAs per 64 B of W), and
// hipBLASLt runs ~50% of the roofline at these M — so the bench's B≈6
// decode steps were paying ~2x on every weight read. GEMM-shaped work
// belongs on the matrix cores: this kernel streams W once through
// v_mfma_f32_16x16x32_bf16 tiles, which makes the arithmetic free and
// leaves pure weight streaming.
//
// Structure: NT (1, 2 or 4) 16-row N-tiles per 4-wave workgroup, all fed
// by one A fragment. Each wave owns a quarter of K (split-K inside the
// workgroup, no global atomics); per k-chunk of 32 and per tile:
//   A-frag: lane (row = lane&15 -> x row m, k = k0 + (lane>>4)*8 + i)
//           — 16 B contiguous per lane; rows m >= M are zero.
//   B-frag: lane (col = lane&15 -> W row n0+(lane&15), same k split)
//           — 16 B contiguous per lane; 4 lanes stride-16 cover a full
//           64 B cacheline of each W row.
//   acc = mfma(a, b, acc)  (C/D: row = (lane>>4)*4 + i, col = lane&15)
// Epilogue: the 4 waves' C tiles reduce through LDS; wave j writes tile j
// as bf16 — or, for a fused gate_up weight, wave 0 applies SwiGLU to the
// (gate, up) tile pair and writes [M, I] directly.
// fp32 accumulation, bf16 I/O — same numeric class as hipBLASLt.

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

#define NWAVES 4  // waves per workgroup = K split factor
#define KSTEP 32  // one mfma k-chunk
#define KUNROLL 4  // k-chunks in flight per iteration

// NT 16-row N-tiles per workgroup share ONE A fragment per k-chunk: with
// a single tile per workgroup every 16 x K weight tile (16*K*2 B from
// HBM) drags the whole M x K activation (M*K*2 B) through L2 -> L1 on the
// same vector-memory path — +50% load traffic at M=8, +100% at M=16.
// Tile j of workgroup b covers W rows b*wg_stride + j*tile_stride + 0..15:
//   plain GEMM : wg_stride = NT*16, tile_stride = 16 (NT adjacent tiles)
//   SwiGLU     : NT = 2, wg_stride = 16, tile_stride = I — the gate tile
//                and its up tile, so the epilogue holds both operands of
//                out[m, n] = silu(gate[m, n]) * up[m, n] and the [M, 2I]
//                intermediate never reaches memory.
// Each output element sees exactly the single-tile arithmetic (same
// per-wave chunk order, same red[0]+red[1]+red[2]+red[3] reduction), so
// results are bit-identical for every NT.
template <int KU, int NT, bool SWIGLU>
__global__ void __launch_bounds__(NWAVES* WAVE)
gemm_skinny_kernel(short* __restrict__ out,      // [M, N] (row stride out_ts)
                   const short* __restrict__ x,  // [M, K] (row stride x_ts)
                   const short* __restrict__ w,  // [N, K]
                   int M, int N, int K, long x_ts, long out_ts,
                   int wg_stride, int tile_stride) {
  static_assert(!SWIGLU || NT == 2, "SwiGLU pairs one gate and one up tile");
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * wg_stride;

  // this wave's K quarter (K % (NWAVES*KSTEP*KUNROLL) checked host-side)
  const int kq = K / NWAVES;
  const int kbeg = wave * kq;
  const int kend = kbeg + kq;

  const int a_row = lane & 15;          // x row (m)
  const int k_off = (lane >> 4) * 8;    // this lane's k sub-offset
  const bool a_live = a_row < M;
  const short* xrow = x + (long)a_row * x_ts;
  // tiles past N (ragged N, or the dead tiles of the last workgroup when
  // the tile count is no multiple of NT) load nothing and store nothing
  bool b_live[NT];
  const short* wrow[NT];
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

  auto load_group = [&](int k0, bf16x8 (&a)[KU], bf16x8 (&b)[NT][KU]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int kk = k0 + u * KSTEP + k_off;
      a[u] = a_live ? *(const bf16x8*)(xrow + kk) : zero8;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        b[j][u] = b_live[j] ? *(const bf16x8*)(wrow[j] + kk) : zero8;
    }
  };
  auto mfma_group = [&](const bf16x8 (&a)[KU], const bf16x8 (&b)[NT][KU]) {
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[j][u], acc[j],
                                                         0, 0, 0);
  };
  for (int k0 = kbeg; k0 < kend; k0 += KSTEP * KU) {
    bf16x8 a[KU], b[NT][KU];
    load_group(k0, a, b);
    mfma_group(a, b);
  }

  // cross-wave reduction: C tiles are [16 m x 16 n] fp32, 1 KB per wave
  // and tile
  __shared__ float red[NT][NWAVES][16][16];
  const int c_col = lane & 15;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[j][wave][(lane >> 4) * 4 + i][c_col] = acc[j][i];
  __syncthreads();
  if constexpr (SWIGLU) {
    // wave 0: reduce the gate and the up tile, round both to bf16 as the
    // plain GEMM's store does, then the silu_mul formula; out is [M, I]
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = (lane >> 4) * 4 + i;
        const int n = n0 + c_col;
        if (m < M && n < tile_stride) {
          float g = red[0][0][m][c_col] + red[0][1][m][c_col] +
                    red[0][2][m][c_col] + red[0][3][m][c_col];
          float u = red[1][0][m][c_col] + red[1][1][m][c_col] +
                    red[1][2][m][c_col] + red[1][3][m][c_col];
          out[(long)m * out_ts + n] = swiglu_bf16(f2bf(g), f2bf(u));
        }
      }
    }
  } else {
    // wave j writes tile j (bf16)
    for (int j = wave; j < NT; j += NWAVES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = (lane >> 4) * 4 + i;
        const int n = n0 + j * tile_stride + c_col;
        if (m < M && n < N) {
          float v = red[j][0][m][c_col] + red[j][1][m][c_col] +
                    red[j][2][m][c_col] + red[j][3][m][c_col];
          out[(long)m * out_ts + n] = f2bf(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Grouped skinny GEMM for MoE decode (capture-safe expert dispatch).
//
// out[p, :] = x[p, :] @ W[e, :, :]^T for rows p in expert e's contiguous
// segment [offsets[e], offsets[e]+counts[e]). Counts/offsets are DEVICE
// tensors — no host-side shapes depend on routing, so a Mixtral decode
// step is hipGraph-capturable (the round-1 masked-gather path called
// nonzero() per expert per layer: a stream sync that aborted capture).
// Each (n-tile, expert) block loops the segment in 16-row chunks; decode
// segments are <= tokens*top_k (<= 32), so expert weights stream at most
// twice.
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(NWAVES* WAVE)
moe_grouped_kernel(short* __restrict__ out,      // [P, N]
                   const short* __restrict__ x,  // [P, K] dense
                   const short* __restrict__ w,  // [E, N, K]
                   const int* __restrict__ counts,   // [E]
                   const int* __restrict__ offsets,  // [E]
                   int N, int K) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * 16;
  const int e = blockIdx.y;
  const int cnt = counts[e];
  if (cnt == 0) return;
  const int off = offsets[e];
  const short* we = w + (long)e * N * K;

  const int kq = K / NWAVES;
  const int kbeg = wave * kq;
  const int kend = kbeg + kq;
  const int a_row = lane & 15;
  const int k_off = (lane >> 4) * 8;
  const int b_row = n0 + (lane & 15);
  const bool b_live = b_row < N;
  const short* wrow = we + (long)b_row * K;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  __shared__ float red[NWAVES][16][16];
  const int c_col = lane & 15;

  for (int mb = 0; mb < cnt; mb += 16) {
    const bool a_live = mb + a_row < cnt;
    const short* xrow = x + (long)(off + mb + a_row) * K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += KSTEP * KUNROLL) {
      bf16x8 a[KUNROLL], b[KUNROLL];
#pragma unroll
      for (int u = 0; u < KUNROLL; ++u) {
        const int kk = k0 + u * KSTEP + k_off;
        a[u] = a_live ? *(const bf16x8*)(xrow + kk) : zero8;
        b[u] = b_live ? *(const bf16x8*)(wrow + kk) : zero8;
      }
#pragma unroll
      for (int u = 0; u < KUNROLL; ++u)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][(lane >> 4) * 4 + i][c_col] = acc[i];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = (lane >> 4) * 4 + i;
        const int n = n0 + c_col;
        if (mb + m < cnt && n < N) {
          float v = red[0][m][c_col] + red[1][m][c_col] + red[2][m][c_col] +
                    red[3][m][c_col];
          out[(long)(off + mb + m) * N + n] = f2bf(v);
        }
      }
    }
    __syncthreads();
  }
}

void moe_grouped_linear(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                        torch::Tensor counts, torch::Tensor offsets) {
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(w.is_contiguous(), "expert weights must be contiguous [E,N,K]");
  TORCH_CHECK(out.is_contiguous());
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 &&
              offsets.scalar_type() == torch::kInt32);
  const int K = x.size(1), E = w.size(0), N = w.size(1);
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16,
              "expert weights must be bfloat16; got ", w.scalar_type());
  TORCH_CHECK(w.dim() == 3 && w.size(2) == K,
              "expert weights must be [E, N, K] with K=", K, "; got ",
              w.sizes());
  TORCH_CHECK(K % (NWAVES * KSTEP * KUNROLL) == 0, "K must be /512");
  const int tiles = (N + 15) / 16;
  hipLaunchKernelGGL(moe_grouped_kernel, dim3(tiles, E), dim3(NWAVES * WAVE),
                     0, c10::hip::getCurrentHIPStream(),
                     (short*)out.data_ptr(), (const short*)x.data_ptr(),
                     (const short*)w.data_ptr(),
                     (const int*)counts.data_ptr(),
                     (const int*)offsets.data_ptr(), N, K);
  HIP_CHECK_LAST();
}

// k-chunks in flight per iteration (KU). Bit-identical either way: the
// per-wave chunk ORDER is the same, only how many loads are issued before
// the first MFMA differs. Measured at M=8 (profiles/
// microbench_skinny_swp_unroll_ab.jsonl): KU=8 takes the deep-K down_proj
// (K=14336, N=4096) from 30.7 to 26.1 us — each wave there walks 28
// chunks and a 256-workgroup grid has no other waves to hide the latency —
// and is flat-to-worse on the K=4096 shapes (qkv 15.2 -> 15.9), so auto is
// 8 for K >= 8192. DTS_SKINNY_UNROLL=4|8 pins it process-wide for A/B;
// unset now means this auto rule (it used to mean 4).
static int skinny_unroll(int K, int64_t unroll) {
  static const int env_ku = [] {
    const char* e = getenv("DTS_SKINNY_UNROLL");
    return (e && e[0] == '8') ? 8 : (e && e[0] == '4') ? 4 : 0;
  }();
  // an explicit unroll=8 on a K that is no multiple of 1024 is an error;
  // the env pin and the auto rule fall back to 4 there
  TORCH_CHECK(unroll != 8 || K % (NWAVES * KSTEP * 8) == 0,
              "unroll=8 needs K % 1024 == 0, got K=", K);
  int ku = unroll ? (int)unroll : env_ku ? env_ku : (K >= 8192 ? 8 : 4);
  if (K % (NWAVES * KSTEP * 8) != 0) ku = 4;
  return ku;
}

#define SKINNY_LAUNCH(KU_, NT_, SW_, grid_, wgs_, ts_)                        \
  hipLaunchKernelGGL((gemm_skinny_kernel<KU_, NT_, SW_>), dim3(grid_),       \
                     dim3(NWAVES * WAVE), 0, stream, (short*)out.data_ptr(), \
                     (const short*)x.data_ptr(), (const short*)w.data_ptr(), \
                     M, N, K, x.stride(0), out.stride(0), wgs_, ts_)

// Tiles per workgroup (NT), measured rule (cold weights, MI355X,
// profiles/microbench_decode_kernels_nt_sweep.jsonl; us at NT=1 -> best):
//   M <= 7          : 1 everywhere — sharing A saves little while fewer,
//                     fatter workgroups cost 2-4 us (gate_up M=4: 44.8 ->
//                     48.9 at NT=2)
//   lm_head  (8016 tiles)  M=8: 215 -> 201 (NT=4), M=16: 280 -> 218
//   gate_up  (1792 tiles)  M=8: flat (51.6/52.4/52.8), M=16: 66 -> 57 (NT=4)
//   qkv      (384 tiles)   M=8: 15.2 -> 14.7 (NT=2), M=16: 18.8 -> 16.3;
//                          NT=4 leaves 96 workgroups: 23 us
//   o / down (256 tiles)   NT=2 halves a one-per-CU grid: +30%, stays 1
// The rule keys on M and the tile count alone and was measured ONLY on
// these five Llama-3-8B shapes. Other (K, N) that reach linear_bf16 — TP
// shards, Mixtral attention projections — fall into the same bands
// unmeasured; the down_proj rows show that deep-K shapes suffer most from
// fewer workgroups, so re-measure before relying on it there.
static int skinny_auto_tiles(int M, int tiles) {
  if (M < 8) return 1;
  if (tiles >= 4096) return 4;
  if (tiles >= 1024) return M > 8 ? 4 : 1;
  if (tiles >= 384) return 2;
  return 1;
}

void gemm_skinny_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                      int64_t tiles_per_wg, int64_t unroll) {
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(w.is_contiguous(), "weight must be contiguous [N, K]");
  TORCH_CHECK(x.stride(1) == 1, "x rows must be dense");
  TORCH_CHECK(out.stride(1) == 1);
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= 16, "skinny path is for M<=16");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16,
              "weight must be bfloat16; got ", w.scalar_type());
  TORCH_CHECK(K % (NWAVES * KSTEP * KUNROLL) == 0, "K must be /512");
  TORCH_CHECK(w.size(1) == K && out.size(0) == M && out.size(1) == N);
  TORCH_CHECK(tiles_per_wg == 0 || tiles_per_wg == 1 || tiles_per_wg == 2 ||
                  tiles_per_wg == 4,
              "tiles_per_wg must be 0 (auto), 1, 2 or 4");
  TORCH_CHECK(unroll == 0 || unroll == 4 || unroll == 8,
              "unroll must be 0 (auto), 4 or 8");
  const int tiles = (N + 15) / 16;
  const int nt =
      tiles_per_wg ? (int)tiles_per_wg : skinny_auto_tiles(M, tiles);
  const int grid = (tiles + nt - 1) / nt;
  auto stream = c10::hip::getCurrentHIPStream();
  if (skinny_unroll(K, unroll) == 8) {
    if (nt == 4) SKINNY_LAUNCH(8, 4, false, grid, 64, 16);
    else if (nt == 2) SKINNY_LAUNCH(8, 2, false, grid, 32, 16);
    else SKINNY_LAUNCH(8, 1, false, grid, 16, 16);
  } else {
    if (nt == 4) SKINNY_LAUNCH(4, 4, false, grid, 64, 16);
    else if (nt == 2) SKINNY_LAUNCH(4, 2, false, grid, 32, 16);
    else SKINNY_LAUNCH(4, 1, false, grid, 16, 16);
  }
  HIP_CHECK_LAST();
}

// out[M, I] = silu(x @ Wg^T) * (x @ Wu^T) with w = [Wg ; Wu] of shape
// [2I, K]: the gate_up projection and the SwiGLU activation in one pass.
void gemm_skinny_swiglu_bf16(torch::Tensor out, torch::Tensor x,
                             torch::Tensor w) {
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(w.is_contiguous(), "weight must be contiguous [2I, K]");
  TORCH_CHECK(x.stride(1) == 1, "x rows must be dense");
  TORCH_CHECK(out.stride(1) == 1);
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  const int I = N / 2;
  TORCH_CHECK(M >= 1 && M <= 16, "skinny path is for M<=16");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16,
              "weight must be bfloat16; got ", w.scalar_type());
  TORCH_CHECK(K % (NWAVES * KSTEP * KUNROLL) == 0, "K must be /512");
  TORCH_CHECK(N == 2 * I && I % 16 == 0, "fused SwiGLU needs I % 16 == 0");
  TORCH_CHECK(w.size(1) == K && out.size(0) == M && out.size(1) == I);
  const int grid = I / 16;
  auto stream = c10::hip::getCurrentHIPStream();
  if (skinny_unroll(K, 0) == 8)
    SKINNY_LAUNCH(8, 2, true, grid, 16, I);
  else
    SKINNY_LAUNCH(4, 2, true, grid, 16, I);
  HIP_CHECK_LAST();
}
#undef SKINNY_LAUNCH
