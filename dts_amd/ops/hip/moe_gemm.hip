// Tiled grouped GEMM for MoE steps past the decode sizes (gfx950).
//
// out[p, :] = x[p, :] @ W[e]^T for every row p of expert e's segment
// [offsets[e], offsets[e] + counts[e]); rows are sorted by expert, counts and
// offsets live in DEVICE memory, so no host-visible shape depends on routing
// and a call is hipGraph-capturable. With SWIGLU, W[e] = [gate; up] ([2I, K])
// and out[p, n] = swiglu_bf16(bf16(x Wg^T), bf16(x Wu^T)): silu_mul of the
// plain result by construction.
//
// moe_grouped_kernel (gemm_skinny.hip) walks a segment 16 rows at a time and
// streams the expert's weights once per pass; this kernel streams a weight
// tile once per 64 rows:
//
//   block     BM = 64 rows x BN = 64 columns, 4 waves. Wave w owns columns
//             n0 + 16w .. +15 and all four 16-row M-tiles: four f32x4
//             accumulators (eight with SwiGLU), each B fragment feeds up to
//             four v_mfma_f32_16x16x32_bf16.
//   weights   global -> registers, never LDS (no other wave needs them):
//             row = lane & 15, 8 consecutive k at (lane >> 4) * 8, one 16 B
//             load, as in the skinny kernels. A ring of MG_PF K-steps is in
//             flight per wave; the loads are branch-free (rows past N and
//             steps past K are clamped to valid addresses: a clamped row only
//             feeds a column that is never stored, a clamped step is never
//             consumed).
//   x         the 64-row block is shared by the four waves: LDS, K-steps of
//             64, double-buffered. Its global loads ride the weights' ring
//             (vector loads complete in issue order, so an x load issued
//             behind a weight load would make its wait drain the ring) and
//             are written to the other buffer behind the step's MFMAs; one
//             barrier per step ends both the reads of buffer s and the writes
//             of buffer s + 1. Row stride 72 bf16 = 144 B = 36 banks: the 16 rows
//             of one ds_read_b128 phase start at banks 36 m mod 64 = 0, 36, 8,
//             44, ... — sixteen distinct multiples of 4 — so the phase covers
//             all 64 banks once (a plain 128 B stride puts them on two bank
//             groups, 8 ways). Rows >= the block's row count are zero in LDS
//             and not read from memory; an M-tile wholly past the segment's
//             end is skipped (workgroup-uniform).
//   sums      one accumulator per output element, ascending k, no split-K:
//             a row's result depends on that row and the expert's weights
//             alone, not on its place in x, its segment's length or its block.
//   block map grid = ceil(N / 64) * (P / 64 + E) workgroups, an upper bound on
//             ceil(N / 64) * sum_e ceil(counts[e] / 64) that needs only
//             shapes. A workgroup walks counts (E <= 64) to find its (expert,
//             column tile, row block), in that order, so the row blocks that
//             share a weight tile are dispatched next to each other; ids past
//             the last block exit. No workspace, no atomics.

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

#define MG_BM 64             // rows per block
#define MG_BN 64             // output columns per block (16 per wave)
#define MG_KS 64             // k per LDS step: two MFMA chunks
#define MG_LDA (MG_KS + 8)   // LDS row stride (bf16): see the header
#define MG_PF 4              // weight K-steps in flight per wave
#define MG_MAX_E 64

template <bool SWIGLU>
__global__ void __launch_bounds__(4 * WAVE)
moe_gemm_kernel(short* __restrict__ out,      // [P, N]
                const short* __restrict__ x,  // [P, K] dense
                const short* __restrict__ w,  // [E, N (SwiGLU: 2N), K]
                const int* __restrict__ counts,   // [E]
                const int* __restrict__ offsets,  // [E]
                int E, int P, int N, int K, int col_tiles) {
  constexpr int NB = SWIGLU ? 2 : 1;  // B fragments per k-chunk
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);

  // ---- block map: (expert, column tile, row block) of this workgroup
  long id = blockIdx.x;
  int e = 0, nblk = 0;
  for (; e < E; ++e) {
    nblk = (min(max(counts[e], 0), P) + MG_BM - 1) / MG_BM;
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
  const int rows = min(min(counts[e], P - off) - mb * MG_BM, MG_BM);
  if (rows <= 0) return;
  const int row0 = off + mb * MG_BM;
  const int m_tiles = (rows + 15) >> 4;
  const int n0 = ct * MG_BN + wave * 16;
  const int nsteps = K / MG_KS;

  // ---- weights: this lane's row of the wave's 16 columns (clamped)
  const int k_off = (lane >> 4) * 8;
  const int b_row = min(n0 + (lane & 15), N - 1);
  const short* wrow[NB];
  wrow[0] = w + ((long)e * (NB * N) + b_row) * K + k_off;
  if (SWIGLU) wrow[NB - 1] = wrow[0] + (long)N * K;

  // ---- x staging: 64 rows x 8 16-byte pieces per step, two per thread
  __shared__ __attribute__((aligned(16))) short sA[2][MG_BM * MG_LDA];
  const short* xsrc[2];
  int xdst[2];
  bool xlive[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int piece = threadIdx.x + j * 4 * WAVE;
    const int r = piece >> 3, kc = (piece & 7) * 8;
    xlive[j] = r < rows;
    xsrc[j] = x + (long)(row0 + min(r, rows - 1)) * K + kc;
    xdst[j] = r * MG_LDA + kc;
  }
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto load_x = [&](bf16x8 (&dst)[2], int step) {
    const int k0 = min(step, nsteps - 1) * MG_KS;
#pragma unroll
    for (int j = 0; j < 2; ++j) dst[j] = *(const bf16x8*)(xsrc[j] + k0);
  };
  auto load_w = [&](bf16x8 (&dst)[2][NB], int step) {
    const int k0 = min(step, nsteps - 1) * MG_KS;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int g = 0; g < NB; ++g)
        dst[c][g] = *(const bf16x8*)(wrow[g] + k0 + c * 32);
  };
  auto store_x = [&](int buf, const bf16x8 (&src)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      *(bf16x8*)&sA[buf][xdst[j]] = xlive[j] ? src[j] : zero8;
  };

  // Rings of MG_PF steps, slot = step % MG_PF: bq[u] holds the weights of
  // step s (s % MG_PF == u), xq[u] the x pieces of step s. Loads complete in
  // issue order, so x rides the same ring as the weights: the issue order is
  // X(1) W(0) X(2) W(1) ..., and waiting for X(s + 1) at the end of step s
  // leaves the weights of steps s + 1 .. s + MG_PF - 1 in flight.
  bf16x8 bq[MG_PF][2][NB], xq[MG_PF][2];
  load_x(xq[0], 0);
#pragma unroll
  for (int d = 0; d < MG_PF; ++d) {
    if (d == 0) store_x(0, xq[0]);
    load_x(xq[(d + 1) % MG_PF], d + 1);
    load_w(bq[d], d);
  }
  __syncthreads();

  f32x4 acc[4][NB];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int g = 0; g < NB; ++g) acc[mt][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int a_off = (lane & 15) * MG_LDA + k_off;
  for (int s0 = 0; s0 < nsteps; s0 += MG_PF) {
#pragma unroll
    for (int u = 0; u < MG_PF; ++u) {
      const int s = s0 + u;
      if (s >= nsteps) break;
      const short* cur = sA[u & 1];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          if (mt < m_tiles) {
            const bf16x8 a =
                *(const bf16x8*)(cur + mt * 16 * MG_LDA + a_off + c * 32);
#pragma unroll
            for (int g = 0; g < NB; ++g)
              acc[mt][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a, bq[u][c][g], acc[mt][g], 0, 0, 0);
          }
      // x of step s + 1 goes to the other buffer (its last readers passed
      // the barrier of step s - 1); both slots are then free for the loads
      // of MG_PF steps ahead. One barrier ends this step's reads and writes.
      store_x((u + 1) & 1, xq[(u + 1) % MG_PF]);
      load_x(xq[(u + 1) % MG_PF], s + 1 + MG_PF);
      load_w(bq[u], s + MG_PF);
      __syncthreads();
    }
  }

  // ---- C: row = mt * 16 + (lane >> 4) * 4 + i, column = lane & 15
  const int n = n0 + (lane & 15);
  if (n >= N) return;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mt * 16 + (lane >> 4) * 4 + i;
      if (m < rows) {
        const short v0 = f2bf(acc[mt][0][i]);
        out[(long)(row0 + m) * N + n] =
            SWIGLU ? swiglu_bf16(v0, f2bf(acc[mt][NB - 1][i])) : v0;
      }
    }
}

// moe_gemm_wide.hip: the 128-row block kernel, same contract
void moe_gemm_wide_launch(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                          torch::Tensor counts, torch::Tensor offsets,
                          bool swiglu);

// Rows per block that auto (block = 0) takes for a call of P rows, the only
// size the host knows without a sync. Measured at the Mixtral-8x7B shapes
// (docs/KERNELS.md, "128-row blocks"): from 1024 rows on the 128-row kernel
// is faster for uniform and skewed routing alike, at 512 rows only for the
// skewed one. Both kernels give the same bits.
static int64_t moe_gemm_auto_block(long P) { return P >= 1024 ? 128 : MG_BM; }

void moe_grouped_gemm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                      torch::Tensor counts, torch::Tensor offsets,
                      bool swiglu, int64_t block) {
  TORCH_CHECK(block == 0 || block == 64 || block == 128,
              "block must be 0 (auto), 64 or 128; got ", block);
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && out.is_cuda() &&
                  counts.is_cuda() && offsets.is_cuda(),
              "moe_grouped_gemm takes device tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.dim() == 2 &&
                  x.is_contiguous(),
              "x must be a contiguous bfloat16 [P, K]");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16,
              "expert weights must be bfloat16; got ", w.scalar_type());
  const long P = x.size(0), K = x.size(1);
  TORCH_CHECK(w.dim() == 3 && w.size(2) == K && w.is_contiguous(),
              "expert weights must be contiguous [E, N, K] with K=", K,
              "; got ", w.sizes());
  const long E = w.size(0), rows_w = w.size(1);
  TORCH_CHECK(E >= 1 && E <= MG_MAX_E, "1 <= E <= 64; got ", E);
  TORCH_CHECK(K > 0 && K % MG_KS == 0, "K must be a multiple of 64; got ", K);
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 &&
                  offsets.scalar_type() == torch::kInt32,
              "counts and offsets must be int32");
  TORCH_CHECK(counts.is_contiguous() && offsets.is_contiguous() &&
                  counts.numel() == E && offsets.numel() == E,
              "counts and offsets must be contiguous [E]");
  TORCH_CHECK(rows_w >= 1 && (!swiglu || rows_w % 32 == 0),
              "SwiGLU weights are [E, 2I, K] with I % 16 == 0; got ",
              w.sizes());
  const long N = swiglu ? rows_w / 2 : rows_w;
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 && out.is_contiguous() &&
                  out.dim() == 2 && out.size(0) == P && out.size(1) == N,
              "out must be a contiguous bfloat16 [", P, ", ", N, "]; got ",
              out.sizes());
  if (P == 0) return;
  if (block == 0) block = moe_gemm_auto_block(P);
  if (block == 128) {
    moe_gemm_wide_launch(out, x, w, counts, offsets, swiglu);
    return;
  }
  const long col_tiles = (N + MG_BN - 1) / MG_BN;
  const long grid = col_tiles * (P / MG_BM + E);
  TORCH_CHECK(P < (1L << 31) - MG_BM && grid < (1L << 31),
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
    launch(moe_gemm_kernel<true>);
  else
    launch(moe_gemm_kernel<false>);
  HIP_CHECK_LAST();
}
