// Wide tiled grouped GEMM for MoE prefill-size steps (gfx950).
//
// The contract of moe_gemm_kernel (moe_gemm.hip): out[p, :] = x[p, :] @ W[e]^T
// for every row p of expert e's segment [offsets[e], offsets[e] + counts[e]),
// rows sorted by expert, counts and offsets int32 in DEVICE memory, rows of no
// segment never written, a segment clipped to x's P rows, K % 64 == 0,
// E <= 64, N ragged; no workspace, no atomics, hipGraph-capturable. With
// SWIGLU, W[e] = [gate; up] ([2I, K]) and out[p, n] =
// swiglu_bf16(bf16(x Wg^T), bf16(x Wu^T)).
//
// moe_gemm_kernel reads a weight tile once per 64 rows, every wave for itself,
// straight from global memory. This kernel reads a weight tile once per 128
// rows and an activation tile once per 128 weight rows, both through LDS and
// shared by all waves:
//
//   block     BM = 128 rows x 128 weight rows, 4 waves arranged 2 x 2. Wave
//             (wm, wn) = (wave >> 1, wave & 1) owns rows 64 wm .. +63 and four
//             16-row weight tiles: 4 M-tiles x 4 N-tiles of
//             v_mfma_f32_16x16x32_bf16, sixteen f32x4 accumulators.
//             Plain: the block's 128 staged weight rows are output columns
//             n0 .. n0 + 127, wave wn owns staged rows 64 wn .. +63.
//             SwiGLU: the block is 64 output columns; staged rows 0..63 are the
//             gate rows n0 + j, 64..127 the up rows I + n0 + j. Wave wn owns
//             output columns n0 + 32 wn .. +31: gate tiles at staged rows
//             32 wn, 32 wn + 16 and up tiles at 64 + 32 wn, 64 + 32 wn + 16, so
//             gate and up of one output meet in one lane.
//   LDS       both operands, K-steps of 64, two stages: 2 x (128 + 128) rows
//             x 72 bf16 x 2 B = 73,728 B, two workgroups per CU. Row stride
//             72 bf16 = 144 B = 36 banks: the 16 lanes of one ds_read_b128
//             phase read rows m = 0..15 at the same k and start at banks
//             36 m mod 64 = 0, 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20,
//             56, 28 -- sixteen distinct multiples of 4, so a phase covers the
//             64 banks once. The weight fragment has the lane layout of the x
//             fragment (row lane & 15, k (lane >> 4) * 8), so the same holds
//             for it. Derived, not counted.
//   loads     per step and thread 4 x 16 B of x and 4 x 16 B of w. The global
//             loads of step s + 1 are issued before step s's MFMAs and written
//             to the other stage after them (issue early, write late); one
//             barrier per step ends the reads of stage s and the writes of
//             stage s + 1. Loads are branch-free: an x row >= the block's row
//             count is clamped to the last valid row and replaced by zero at
//             the LDS write; a weight row >= N is clamped to N - 1 and only
//             feeds a column that is never stored.
//   edges     an M-tile wholly past the segment's end is skipped, wave-
//             uniformly; a wave whose 64-row half is empty still stages its
//             share and reaches every barrier. Columns >= N are not stored.
//   sums      one accumulator per output element, ascending 32-k chunks, x is
//             the A operand and w the B operand with moe_gemm_kernel's lane
//             layout: every output is bit-identical to moe_gemm_kernel's.
//   block map grid = col_tiles * (P / 128 + E), col_tiles = ceil(N / 128)
//             (SwiGLU: ceil(N / 64)). A workgroup walks counts to its (expert,
//             column tile, row block), in that order, so the row blocks that
//             share a weight tile are dispatched next to each other; ids past
//             the last block exit.

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

#define MW_BM 128            // rows per block (two wave rows of 64)
#define MW_BW 128            // staged weight rows per block
#define MW_KS 64             // k per LDS step: two MFMA chunks
#define MW_LD (MW_KS + 8)    // LDS row stride (bf16): see the header
#define MW_PIECES 4          // 16 B pieces per thread, step and operand

template <bool SWIGLU>
__global__ void __launch_bounds__(4 * WAVE, 2)
moe_gemm_wide_kernel(short* __restrict__ out,      // [P, N]
                     const short* __restrict__ x,  // [P, K] dense
                     const short* __restrict__ w,  // [E, N (SwiGLU: 2N), K]
                     const int* __restrict__ counts,   // [E]
                     const int* __restrict__ offsets,  // [E]
                     int E, int P, int N, int K, int col_tiles) {
  constexpr int BM = MW_BM;
  constexpr int BN = SWIGLU ? MW_BW / 2 : MW_BW;  // output columns per block
  // wave-uniform by construction; in a scalar register so that the M-tile
  // skips below are scalar branches
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- block map: (expert, column tile, row block) of this workgroup
  long id = blockIdx.x;
  int e = 0, nblk = 0;
  for (; e < E; ++e) {
    nblk = (min(max(counts[e], 0), P) + BM - 1) / BM;
    const long span = (long)nblk * col_tiles;
    if (id < span) break;
    id -= span;
  }
  if (e == E) return;
  const int ct = (int)(id / nblk);
  const int mb = (int)(id - (long)ct * nblk);
  const int off = offsets[e];
  if (off < 0) return;
  // a segment never reaches past x, whatever counts and offsets say
  const int rows = min(min(counts[e], P - off) - mb * BM, BM);
  if (rows <= 0) return;
  const int row0 = off + mb * BM;
  const int n0 = ct * BN;
  const int nsteps = K / MW_KS;
  // M-tiles of this wave's 64-row half that hold a row of the segment
  const int m_tiles = (min(max(rows - wm * 64, 0), 64) + 15) >> 4;

  // ---- staging: 128 rows x 8 16-byte pieces per operand and step
  __shared__ __attribute__((aligned(16))) short sX[2][BM * MW_LD];
  __shared__ __attribute__((aligned(16))) short sW[2][MW_BW * MW_LD];
  const short* xsrc[MW_PIECES];
  const short* wsrc[MW_PIECES];
  int dst[MW_PIECES];
  bool xlive[MW_PIECES];
  const short* wexp = w + (long)e * (SWIGLU ? 2 : 1) * N * K;
#pragma unroll
  for (int j = 0; j < MW_PIECES; ++j) {
    const int piece = threadIdx.x + j * 4 * WAVE;
    const int r = piece >> 3, kc = (piece & 7) * 8;
    xlive[j] = r < rows;
    xsrc[j] = x + (long)(row0 + min(r, rows - 1)) * K + kc;
    // staged weight row r: column n0 + r (SwiGLU: gate n0 + r for r < 64,
    // up I + n0 + r - 64 above), clamped to the last column
    const int wr = SWIGLU ? (r >> 6) * N + min(n0 + (r & 63), N - 1)
                          : min(n0 + r, N - 1);
    wsrc[j] = wexp + (long)wr * K + kc;
    dst[j] = r * MW_LD + kc;
  }
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 xq[MW_PIECES], wq[MW_PIECES];
  auto load = [&](int step) {
    const int k0 = step * MW_KS;
#pragma unroll
    for (int j = 0; j < MW_PIECES; ++j) xq[j] = *(const bf16x8*)(xsrc[j] + k0);
#pragma unroll
    for (int j = 0; j < MW_PIECES; ++j) wq[j] = *(const bf16x8*)(wsrc[j] + k0);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < MW_PIECES; ++j) {
      *(bf16x8*)&sX[buf][dst[j]] = xlive[j] ? xq[j] : zero8;
      *(bf16x8*)&sW[buf][dst[j]] = wq[j];
    }
  };

  load(0);
  store(0);
  __syncthreads();

  f32x4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment lane layout: row lane & 15, 8 consecutive k at (lane >> 4) * 8
  const int frag = (lane & 15) * MW_LD + (lane >> 4) * 8;
  const int a_off = wm * 64 * MW_LD + frag;
  // staged row of this wave's N-tile nt
  int b_off[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int br = SWIGLU ? (nt >> 1) * 64 + wn * 32 + (nt & 1) * 16
                          : wn * 64 + nt * 16;
    b_off[nt] = br * MW_LD + frag;
  }

  // One K-step of this wave: per 32-k chunk four B and up to four A
  // fragments, each A fragment feeds four MFMAs. FULL: all four M-tiles,
  // no branch between the LDS reads and the MFMAs; the same operations per
  // accumulator either way.
  auto mfma_step = [&](auto full, const short* curx, const short* curw) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      bf16x8 b[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        b[nt] = *(const bf16x8*)(curw + b_off[nt] + c * 32);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        if (decltype(full)::value || mt < m_tiles) {
          const bf16x8 a =
              *(const bf16x8*)(curx + a_off + mt * 16 * MW_LD + c * 32);
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, b[nt], acc[mt][nt], 0, 0, 0);
        }
    }
  };

  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;  // workgroup-uniform
    if (more) load(s + 1);
    if (m_tiles == 4)
      mfma_step(std::true_type{}, sX[s & 1], sW[s & 1]);
    else
      mfma_step(std::false_type{}, sX[s & 1], sW[s & 1]);
    // step s + 1 goes to the other stage: its last readers passed the barrier
    // of step s - 1. One barrier ends this step's reads and those writes.
    if (more) store((s + 1) & 1);
    __syncthreads();
  }

  // ---- C: row = mt * 16 + (lane >> 4) * 4 + i, column = lane & 15
  constexpr int NT_OUT = SWIGLU ? 2 : 4;  // output tiles per wave
#pragma unroll
  for (int nt = 0; nt < NT_OUT; ++nt) {
    const int n = n0 + wn * (NT_OUT * 16) + nt * 16 + (lane & 15);
    if (n >= N) continue;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = wm * 64 + mt * 16 + (lane >> 4) * 4 + i;
        if (m < rows) {
          const short v0 = f2bf(acc[mt][nt][i]);
          out[(long)(row0 + m) * N + n] =
              SWIGLU ? swiglu_bf16(v0, f2bf(acc[mt][(nt + 2) & 3][i])) : v0;
        }
      }
  }
}

// Launch for moe_grouped_gemm(block = 128), which has checked the arguments.
void moe_gemm_wide_launch(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                          torch::Tensor counts, torch::Tensor offsets,
                          bool swiglu) {
  const long P = x.size(0), K = x.size(1), E = w.size(0);
  const long N = out.size(1);
  const long col_tiles = swiglu ? (N + MW_BW / 2 - 1) / (MW_BW / 2)
                                : (N + MW_BW - 1) / MW_BW;
  const long grid = col_tiles * (P / MW_BM + E);
  TORCH_CHECK(P < (1L << 31) - MW_BM && grid < (1L << 31),
              "problem too large");
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(4 * WAVE), 0,
                       c10::hip::getCurrentHIPStream(),
                       (short*)out.data_ptr(), (const short*)x.data_ptr(),
                       (const short*)w.data_ptr(),
                       (const int*)counts.data_ptr(),
                       (const int*)offsets.data_ptr(), (int)E, (int)P, (int)N,
                       (int)K, (int)col_tiles);
  };
  if (swiglu)
    launch(moe_gemm_wide_kernel<true>);
  else
    launch(moe_gemm_wide_kernel<false>);
  HIP_CHECK_LAST();
}
