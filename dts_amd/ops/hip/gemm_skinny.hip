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
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <atomic>

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
// Persistent form: one 16-wave workgroup per CU, activation staged in LDS.
//
// gemm_skinny_kernel pulls the whole M x K activation through L2 -> L1 once
// per workgroup, on the same vector-memory path as the weights (gate_up at
// M=8: 896 x 64 KB = 57 MB beside 235 MB of W). Here a workgroup copies
// x[M, K] into LDS ONCE and then walks its share of the tiles with only
// weight loads on the vector-memory path; A fragments are one 16 B LDS read
// per lane and chunk.
//
// The workgroup is PERSIST_T teams of NWAVES waves; a team is
// gemm_skinny_kernel's workgroup unchanged: wave w owns K-quarter w, walks
// its 32-k chunks in ascending order into one accumulator per tile, and the
// four partials are summed wave0 + wave1 + wave2 + wave3 (wave 0 keeps its
// own partial in registers, which is the same left-to-right sum as
// red[0]+red[1]+red[2]+red[3]) before ONE f2bf — so every output element is
// bit-identical to gemm_skinny_kernel's.
//
// Unit u is one N-tile (W rows 16u..16u+15) or, for SwiGLU, the gate tile
// u and its up tile (rows I + 16u..). Slot s = trip * PERSIST_T + team of
// workgroup b owns unit s * gridDim.x + b: static, no cross-workgroup
// dependency, and every workgroup gets the same number of units +-1.
// Barriers are workgroup-wide, so every team runs the same `trips` loop
// trips; a team without a unit loads and stores nothing.
//
// LDS image: row m at short offset m * (K + 8). Rows >= M are never
// written or read (their A fragment is zero). K % 512 == 0 makes the plain
// 2K-byte row stride a multiple of 1024 B, i.e. all 16 rows of a fragment
// read would hit the same banks (16-way conflict); the 16 B pad shifts row
// m by 4 banks, so the 16 lanes of one ds_read_b128 phase (rows 0..15, same
// k) cover 16 x 16 B = all 64 banks exactly once: 0 conflicts, derived.
// Budget at K = 4096: 16 x 4104 x 2 = 131,328 B image + 24 KB reduction
// (plain: 2 buffers x 4 teams x 3 waves x 1 KB, one barrier per trip;
// SwiGLU: 1 buffer x 4 teams x 2 tiles x 3 waves x 1 KB, two barriers) =
// 155,904 B of the CU's 160 KB.
// ---------------------------------------------------------------------------

#define PERSIST_T 4        // teams per workgroup
#define PERSIST_KMAX 4096  // largest K whose image fits
#define PERSIST_PAD 8      // bf16 of padding per image row
// byte offset a lane without a W row loads from; W must end at or below it
#define PERSIST_DEAD_OFF 0x80000000u

template <int KU, bool SWIGLU>
__global__ void __launch_bounds__(PERSIST_T* NWAVES* WAVE)
gemm_skinny_persistent_kernel(short* __restrict__ out,      // [M, N | I]
                              const short* __restrict__ x,  // [M, K]
                              const short* __restrict__ w,  // [N, K]
                              int M, int N, int K, long x_ts, long out_ts,
                              int units, int tile_stride) {
  constexpr int NT = SWIGLU ? 2 : 1;
  constexpr int NBUF = SWIGLU ? 1 : 2;
  __shared__ __attribute__((aligned(16))) short
      ximg[16 * (PERSIST_KMAX + PERSIST_PAD)];
  __shared__ float red[NBUF][PERSIST_T][NT][NWAVES - 1][16][16];

  const int team = threadIdx.x / (NWAVES * WAVE);
  const int wave = (threadIdx.x / WAVE) % NWAVES;
  const int lane = threadIdx.x & (WAVE - 1);
  const int ld = K + PERSIST_PAD;
  const int slots = gridDim.x * PERSIST_T;
  const int trips = (units + slots - 1) / slots;

  const int kq = K / NWAVES;
  const int kbeg = wave * kq;
  const int kend = kbeg + kq;
  const int a_row = lane & 15;
  const int k_off = (lane >> 4) * 8;
  const bool a_live = a_row < M;
  const short* arow = ximg + a_row * ld;
  const int c_col = lane & 15;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // Weights come through a raw buffer resource over W: a lane without a
  // row (dead unit, row >= N) gets the offset DEAD, which lies past the
  // buffer, so the hardware's range check returns zero for it instead of
  // loading. That keeps the load stream free of branches, so the compiler
  // can count loads in flight and wait for the older group only. The host
  // checks N * K * 2 <= PERSIST_DEAD_OFF: every live offset is below DEAD,
  // and DEAD plus any k offset (< 2 * PERSIST_KMAX + 64 bytes) stays below
  // 2^32, so a dead lane's offset never wraps back into the buffer.
  const __amdgpu_buffer_rsrc_t wbuf = __builtin_amdgcn_make_buffer_rsrc(
      (void*)w, 0, (int)((unsigned)N * (unsigned)K * 2u), 0x00020000);
  constexpr unsigned DEAD = PERSIST_DEAD_OFF;
  int n0 = 0;
  bool u_live = false;
  unsigned woff[NT];  // byte offset of this lane's W row, or DEAD
  auto set_unit = [&](int trip) __attribute__((always_inline)) {
    const int u = (trip * PERSIST_T + team) * gridDim.x + blockIdx.x;
    u_live = trip < trips && u < units;
    n0 = u * 16;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int b_row = n0 + j * tile_stride + (lane & 15);
      woff[j] = (u_live && b_row < N)
                    ? (unsigned)b_row * (unsigned)K * 2u + k_off * 2u
                    : DEAD;
    }
  };
  auto load_b = [&](int k0, bf16x8 (&b)[NT][KU])
                    __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const unsigned off = woff[j] + (unsigned)(k0 + u * KSTEP) * 2u;
        b[j][u] = __builtin_bit_cast(
            bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wbuf, off, 0, 0));
      }
  };

  // Stage x: every load is issued before the first LDS write (at most
  // 16 * PERSIST_KMAX / 8 vectors over 1024 threads = 8 per thread), and
  // the first unit's first weight group is issued behind them, so it
  // stays in flight while the image is written.
  constexpr int NTHREADS = PERSIST_T * NWAVES * WAVE;
  constexpr int NSTAGE = 16 * PERSIST_KMAX / 8 / NTHREADS;
  const int kvec = K / 8;
  bf16x8 st[NSTAGE];
#pragma unroll
  for (int i = 0; i < NSTAGE; ++i) {
    const int v = threadIdx.x + i * NTHREADS;
    const int m = v / kvec, c = (v - m * kvec) * 8;
    st[i] = v < M * kvec ? *(const bf16x8*)(x + (long)m * x_ts + c) : zero8;
  }
  bf16x8 b0[NT][KU], b1[NT][KU];
  set_unit(0);
  load_b(kbeg, b0);
#pragma unroll
  for (int i = 0; i < NSTAGE; ++i) {
    const int v = threadIdx.x + i * NTHREADS;
    const int m = v / kvec, c = (v - m * kvec) * 8;
    if (v < M * kvec) *(bf16x8*)(ximg + m * ld + c) = st[i];
  }
  __syncthreads();

  // One flat loop over every weight group of every trip, two groups in
  // flight: while group g is consumed from `cur`, group g + 1 — of the same
  // unit, or the first of the team's next unit, which then flies over the
  // reduction — is already loading into `nxt`. The two buffers swap roles
  // by calling step() with them exchanged, not by copying.
  constexpr int GROUP = KSTEP * KU;
  const int ngroups = kq / GROUP;
  const int total = trips * ngroups;
  int cur_n0 = n0;
  bool cur_live = u_live;
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};

  auto step = [&](int kg, int trip, const bf16x8 (&cur)[NT][KU],
                  bf16x8 (&nxt)[NT][KU]) __attribute__((always_inline)) {
    const bool last = kg + 1 == ngroups;
    const int k0 = kbeg + kg * GROUP;
    if (last) set_unit(trip + 1);
    load_b(last ? kbeg : k0 + GROUP, nxt);
    bf16x8 a[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u)
      a[u] = a_live ? *(const bf16x8*)(arow + k0 + u * KSTEP + k_off) : zero8;
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], cur[j][u],
                                                         acc[j], 0, 0, 0);
    if (!last) return;
    // the unit is complete: reduce the team's four partials and store
    const int buf = trip & (NBUF - 1);
    if (wave != 0) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          red[buf][team][j][wave - 1][(lane >> 4) * 4 + i][c_col] = acc[j][i];
    }
    __syncthreads();
    if (wave == 0 && cur_live) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = (lane >> 4) * 4 + i;
        float v[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
          v[j] = acc[j][i] + red[buf][team][j][0][m][c_col] +
                 red[buf][team][j][1][m][c_col] +
                 red[buf][team][j][2][m][c_col];
        const int n = cur_n0 + c_col;
        if constexpr (SWIGLU) {
          if (m < M && n < tile_stride)
            out[(long)m * out_ts + n] = swiglu_bf16(f2bf(v[0]), f2bf(v[1]));
        } else {
          if (m < M && n < N) out[(long)m * out_ts + n] = f2bf(v[0]);
        }
      }
    }
    // one reduction buffer: it is rewritten next trip, so readers finish
    // first; with two, the barrier of trip t+1 already orders trip t's
    // reads before trip t+2's writes
    if constexpr (NBUF == 1) __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};
    cur_n0 = n0;
    cur_live = u_live;
  };
  for (int g = 0, kg = 0, trip = 0; g < total; g += 2) {
    step(kg, trip, b0, b1);
    if (++kg == ngroups) kg = 0, ++trip;
    if (g + 1 < total) {
      step(kg, trip, b1, b0);
      if (++kg == ngroups) kg = 0, ++trip;
    }
  }
}

// ---------------------------------------------------------------------------
// Stream form: gemm_skinny_kernel's workgroup with a deep ring of loads.
//
// o, qkv and down have one 4-wave workgroup per CU or fewer: one wave per
// SIMD, nothing else to hide a wait, and gemm_skinny_kernel loads a group
// of KU chunks, uses all of them, then loads the next — the bytes a wave
// has in flight (KU KB) bound its rate. Here wave w keeps a ring of NG
// groups of GC chunks in flight over its K-quarter: the prologue requests
// NG groups; a step waits for the OLDEST group only, runs its MFMAs and
// requests the group NG ahead into the registers it has just freed. The
// ring positions are unrolled, so the register arrays are indexed
// statically and nothing is copied. Nothing is requested past the
// quarter's end.
//
// The arithmetic per output element is gemm_skinny_kernel's: wave w owns
// K-quarter w, its 32-k chunks go in ascending order into ONE accumulator
// per tile, the partials are summed red[0]+red[1]+red[2]+red[3] and
// rounded once — bit-identical.
//
// W and x both come through raw buffer resources, as W does in the
// persistent kernel: a lane without a row (W row >= N, x row >= M) gets
// the offset STREAM_DEAD_OFF, which lies at or past the end of either
// buffer, so the range check returns zero for it and the load stream has
// no branch; only then can the compiler count the loads in flight and
// wait with a non-zero vmcnt. The host checks that W and the x view are
// at most 2 GiB each: every live offset is then below the dead one, and
// the dead one plus any k offset (< 2 K bytes <= 2 GiB) stays below 2^32.
// ---------------------------------------------------------------------------

#define STREAM_GC 8  // chunks per group: the host needs K % 1024 == 0
#define STREAM_DEAD_OFF 0x80000000u

template <int GC, int NG, int NT>
__global__ void __launch_bounds__(NWAVES* WAVE)
gemm_skinny_stream_kernel(short* __restrict__ out,      // [M, N] (out_ts)
                          const short* __restrict__ x,  // [M, K] (x_ts)
                          const short* __restrict__ w,  // [N, K]
                          int M, int N, int K, long x_ts, long out_ts,
                          int wg_stride, int tile_stride) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * wg_stride;
  const int kq = K / NWAVES;
  const int kbeg = wave * kq;
  const int a_row = lane & 15;
  const int k_off = (lane >> 4) * 8;

  const __amdgpu_buffer_rsrc_t wbuf = __builtin_amdgcn_make_buffer_rsrc(
      (void*)w, 0, (int)((unsigned)N * (unsigned)K * 2u), 0x00020000);
  // the x view ends with row M-1; rows past it are outside the resource
  const __amdgpu_buffer_rsrc_t xbuf = __builtin_amdgcn_make_buffer_rsrc(
      (void*)x, 0, (int)(unsigned)(((long)(M - 1) * x_ts + K) * 2), 0x00020000);
  constexpr unsigned DEAD = STREAM_DEAD_OFF;
  // byte offsets of this lane's x row and W rows at the quarter's start
  const unsigned kb0 = (unsigned)(kbeg + k_off) * 2u;
  const unsigned xoff =
      a_row < M ? (unsigned)((long)a_row * x_ts * 2) + kb0 : DEAD;
  unsigned woff[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int b_row = n0 + j * tile_stride + (lane & 15);
    woff[j] = b_row < N ? (unsigned)b_row * (unsigned)K * 2u + kb0 : DEAD;
  }

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};

  constexpr int GROUP = KSTEP * GC;
  const int ngroups = kq / GROUP;
  auto issue = [&](int g, bf16x8 (&a)[GC], bf16x8 (&b)[NT][GC])
                   __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < GC; ++u) {
      const unsigned kb = (unsigned)(g * GROUP + u * KSTEP) * 2u;
      a[u] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(xbuf, xoff + kb, 0, 0));
#pragma unroll
      for (int j = 0; j < NT; ++j)
        b[j][u] = __builtin_bit_cast(
            bf16x8,
            __builtin_amdgcn_raw_buffer_load_b128(wbuf, woff[j] + kb, 0, 0));
    }
  };
  auto consume = [&](const bf16x8 (&a)[GC], const bf16x8 (&b)[NT][GC])
                     __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < GC; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[j][u], acc[j],
                                                         0, 0, 0);
  };

  bf16x8 a[NG][GC], b[NG][NT][GC];
  if (ngroups >= NG) {
#pragma unroll
    for (int r = 0; r < NG; ++r) issue(r, a[r], b[r]);
    // steady state, free of branches: every step refills its ring position
    int g = 0;
    for (; g + 2 * NG <= ngroups; g += NG) {
#pragma unroll
      for (int r = 0; r < NG; ++r) {
        consume(a[r], b[r]);
        issue(g + r + NG, a[r], b[r]);
      }
    }
    // NG .. 2 NG - 1 groups are left and the last NG of them are in flight:
    // the first steps still refill, the rest drain the ring
#pragma unroll
    for (int t = 0; t < 2 * NG - 1; ++t) {
      if (g + t < ngroups) {
        consume(a[t % NG], b[t % NG]);
        if (g + t + NG < ngroups) issue(g + t + NG, a[t % NG], b[t % NG]);
      }
    }
  } else {
    // a quarter shorter than the ring: request all of it, then use it
#pragma unroll
    for (int r = 0; r < NG - 1; ++r)
      if (r < ngroups) issue(r, a[r], b[r]);
#pragma unroll
    for (int r = 0; r < NG - 1; ++r)
      if (r < ngroups) consume(a[r], b[r]);
  }

  // gemm_skinny_kernel's reduction and store
  __shared__ float red[NT][NWAVES][16][16];
  const int c_col = lane & 15;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[j][wave][(lane >> 4) * 4 + i][c_col] = acc[j][i];
  __syncthreads();
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
// unset now means this auto rule (it used to mean 4). 16 and 32 there name
// the stream kernel (skinny_stream_chunks below) and leave this kernel on
// its auto rule.
static int skinny_env_unroll() {
  static const int env_ku = [] {
    const char* e = getenv("DTS_SKINNY_UNROLL");
    const int n = e ? atoi(e) : 0;
    return (n == 4 || n == 8 || n == 16 || n == 32) ? n : 0;
  }();
  return env_ku;
}

static int skinny_unroll(int K, int64_t unroll) {
  const int env_ku = skinny_env_unroll() <= 8 ? skinny_env_unroll() : 0;
  // an explicit unroll=8 on a K that is no multiple of 1024 is an error;
  // the env pin and the auto rule fall back to 4 there
  TORCH_CHECK(unroll != 8 || K % (NWAVES * KSTEP * 8) == 0,
              "unroll=8 needs K % 1024 == 0, got K=", K);
  int ku = unroll ? (int)unroll : env_ku ? env_ku : (K >= 8192 ? 8 : 4);
  if (K % (NWAVES * KSTEP * 8) != 0) ku = 4;
  return ku;
}

// Measured rule for the stream kernel: chunks in flight per wave (and the
// tiles per workgroup in *nt) where it beats the current auto path by more
// than 3x the larger spread, else 0. Cold weights cycled past the Infinity
// Cache, MI355X, 256 CUs, profiles/microbench_skinny_stream.jsonl; current
// auto path -> stream, us, median of 5 alternating rounds, every spread
// <= 0.1:
//   o (K=4096, 256 tiles), 16 chunks, NT=1:
//                 M=1 10.1 -> 7.6, M=4 10.6 -> 8.3, M=6 10.6 -> 8.4,
//                 M=8 10.8 -> 8.6, M=16 11.4 -> 10.0 (32 chunks: 9.8, no
//                 clear difference)
//   qkv (K=4096, 384 tiles), 16 chunks, NT=2 (NT=1 gains <= 0.3 below M=16
//                 and loses there):
//                 M=1 12.0 -> 11.9: no; M=4 13.4 -> 12.5, M=6 14.0 -> 12.8,
//                 M=8 14.6 -> 13.4, M=16 16.1 -> 14.9
//   down (K=14336, 256 tiles), 16 chunks, NT=1:
//                 M=1 23.7 -> 21.7, M=4 24.3 -> 23.5; M=6 24.8 -> 24.6,
//                 M=8 26.0 -> 26.1, M=16 31.4 -> 32.0: no
// 32 chunks in flight never beat 16 by more than the spread (qkv: 1 us
// slower), so the rule does not select them. Only these three (K, tile
// count) pairs were timed, so nothing else is selected; M between the
// measured points takes the band of the next lower one.
static int skinny_auto_tiles(int M, int tiles);

static int skinny_stream_rule(int M, int K, int tiles, int* nt) {
  *nt = 1;
  if (K == 4096 && tiles == 256) return 16;
  if (K == 4096 && tiles == 384 && M >= 4) return *nt = 2, 16;
  if (K == 14336 && tiles == 256 && M < 6) return 16;
  return 0;
}

// Tiles per workgroup the stream kernel is built with at `chunks` in
// flight: 32 chunks of two tiles are 96 loads, and a wave counts 64.
static int skinny_stream_max_tiles(int chunks) { return chunks == 16 ? 2 : 1; }

// Chunks in flight per wave if this call takes the stream kernel, else 0.
// unroll=16|32 pins it, and is an error where K, tiles_per_wg or the buffer
// sizes do not fit; DTS_SKINNY_UNROLL=16|32 and the measured rule apply to
// calls that pin neither unroll nor tiles_per_wg, and fall back to
// gemm_skinny_kernel where something does not fit. *nt is the tiles per
// workgroup: the pinned value, the rule's, or under the env pin what
// skinny_auto_tiles picks as far as the variant exists.
static int skinny_stream_chunks(int64_t unroll, int64_t tiles_per_wg, int M,
                                int N, int K, int tiles, long x_ts, int* nt) {
  const bool k_ok = K % (NWAVES * KSTEP * STREAM_GC) == 0;
  // both buffers are addressed by 32-bit offsets that must stay below the
  // one dead lanes use
  const bool fits =
      (int64_t)N * K * 2 <= (int64_t)STREAM_DEAD_OFF &&
      ((int64_t)(M - 1) * x_ts + K) * 2 <= (int64_t)STREAM_DEAD_OFF;
  if (unroll == 16 || unroll == 32) {
    TORCH_CHECK(k_ok, "unroll=", unroll, " needs K % 1024 == 0, got K=", K);
    TORCH_CHECK(tiles_per_wg <= skinny_stream_max_tiles((int)unroll),
                "unroll=", unroll, " has no tiles_per_wg=", tiles_per_wg,
                " variant");
    TORCH_CHECK(fits, "unroll=", unroll,
                " needs a weight and an x view of at most 2 GiB each");
    *nt = tiles_per_wg ? (int)tiles_per_wg
                       : std::min(skinny_auto_tiles(M, tiles),
                                  skinny_stream_max_tiles((int)unroll));
    return (int)unroll;
  }
  if (unroll != 0 || tiles_per_wg != 0 || !k_ok || !fits) return 0;
  const int env = skinny_env_unroll();
  if (!env) return skinny_stream_rule(M, K, tiles, nt);
  if (env <= 8) return 0;
  *nt = std::min(skinny_auto_tiles(M, tiles), skinny_stream_max_tiles(env));
  return env;
}

#define SKINNY_LAUNCH(KU_, NT_, SW_, grid_, wgs_, ts_)                        \
  hipLaunchKernelGGL((gemm_skinny_kernel<KU_, NT_, SW_>), dim3(grid_),       \
                     dim3(NWAVES * WAVE), 0, stream, (short*)out.data_ptr(), \
                     (const short*)x.data_ptr(), (const short*)w.data_ptr(), \
                     M, N, K, x.stride(0), out.stride(0), wgs_, ts_)

#define STREAM_LAUNCH(NG_, NT_, grid_, wgs_)                                  \
  hipLaunchKernelGGL((gemm_skinny_stream_kernel<STREAM_GC, NG_, NT_>),       \
                     dim3(grid_), dim3(NWAVES* WAVE), 0, stream,             \
                     (short*)out.data_ptr(), (const short*)x.data_ptr(),     \
                     (const short*)w.data_ptr(), M, N, K, x.stride(0),       \
                     out.stride(0), wgs_, 16)

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

// Whether a call takes the persistent kernel. `persistent` is the binding's
// pin (-1 auto, 0 off, 1 on); DTS_SKINNY_PERSISTENT=0|1 pins it process-wide
// for A/B runs; unset means the measured rule. An explicit pin on a K whose
// LDS image does not fit is an error; the env pin and the rule fall back to
// gemm_skinny_kernel there, and so does a call that pins tiles_per_wg or
// unroll, which name that kernel's variants.
//
// Measured rule (cold weights cycled past the Infinity Cache, MI355X, 256
// CUs, profiles/microbench_skinny_persistent.jsonl; current auto path ->
// persistent, us, median of 5 alternating rounds, spreads <= 1.0): the
// persistent path is taken only where it wins by more than 3x the larger
// spread.
//   lm_head (8016 tiles)  M=1 169.3 -> 174.0, M=4 184.5 -> 178.9,
//                         M=8 204.5 -> 184.8, M=16 223.3 -> 195.0
//   gate_up (1792 tiles)  M=1 40.4 -> 43.0, M=4 44.4 -> 44.4,
//                         M=8 52.0 -> 44.2, M=16 56.9 -> 45.2
//   gate_up SwiGLU (896 pairs)  M=1 45.8 -> 44.0, M=4 48.9 -> 45.0,
//                         M=8 52.7 -> 46.0, M=16 59.9 -> 47.1
//   qkv (384 tiles)       M=1 12.6 -> 13.9, M=4 13.5 -> 14.0,
//                         M=8 14.8 -> 15.1, M=16 16.2 -> 16.4: never —
//                         1.5 tiles per CU leave half the teams idle
// Only these K=4096 shapes were timed, and at a smaller K the fixed cost of
// staging and of the barriers weighs more, so the rule selects nothing at
// another K and no unit count below the one measured; M between the
// measured points takes the band of the next lower one.
static bool skinny_persistent_rule(int M, int K, int units, bool swiglu) {
  if (K != 4096) return false;
  if (swiglu) return units >= 896;
  if (units >= 8016) return M >= 4;
  if (units >= 1792) return M >= 8;
  return false;
}

// Process-wide pin: -1 the measured rule, 0 off, 1 on. A knob for tests and
// A/B runs, not for tuning: 1 sends EVERY skinny GEMM whose K fits through
// the persistent kernel, qkv and o_proj included, which lose there. It
// starts from
// DTS_SKINNY_PERSISTENT and can be changed with skinny_persistent_pin(), so
// one process can run both paths (a captured graph keeps the kernel it
// was captured with).
static std::atomic<int> g_persist_pin{[] {
  const char* e = getenv("DTS_SKINNY_PERSISTENT");
  return (e && e[0] == '1') ? 1 : (e && e[0] == '0') ? 0 : -1;
}()};

int64_t skinny_persistent_pin(int64_t pin) {
  TORCH_CHECK(pin >= -1 && pin <= 1, "pin must be -1 (rule), 0 or 1");
  return g_persist_pin.exchange((int)pin);
}

static bool skinny_use_persistent(int64_t persistent, bool other_pins, int M,
                                  int N, int K, int units, bool swiglu) {
  const int env_p = g_persist_pin.load();
  TORCH_CHECK(persistent >= -1 && persistent <= 1,
              "persistent must be -1 (auto), 0 or 1");
  // the image lives in LDS, and W is addressed by 32-bit buffer offsets
  // that must stay below the one dead lanes use
  const bool fits =
      K <= PERSIST_KMAX && (int64_t)N * K * 2 <= (int64_t)PERSIST_DEAD_OFF;
  TORCH_CHECK(persistent != 1 || fits, "persistent=1 needs K <= ",
              PERSIST_KMAX, " and a weight of at most 2 GiB, got K=", K, " N=", N);
  if (persistent >= 0) return persistent == 1;
  if (other_pins || !fits) return false;
  if (env_p >= 0) return env_p == 1;
  return skinny_persistent_rule(M, K, units, swiglu);
}

// The grid is one workgroup per CU: 1024 threads and 156 KB of LDS leave
// room for no second one, and the static tile map is balanced on that
// assumption only (nothing breaks otherwise: workgroups do not depend on
// each other).
#define PERSIST_LAUNCH(KU_, SW_, units_, ts_)                                \
  hipLaunchKernelGGL(                                                        \
      (gemm_skinny_persistent_kernel<KU_, SW_>),                             \
      dim3(at::cuda::getCurrentDeviceProperties()->multiProcessorCount),     \
      dim3(PERSIST_T* NWAVES* WAVE), 0, stream, (short*)out.data_ptr(),      \
      (const short*)x.data_ptr(), (const short*)w.data_ptr(), M, N, K,       \
      x.stride(0), out.stride(0), units_, ts_)

void gemm_skinny_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                      int64_t tiles_per_wg, int64_t unroll,
                      int64_t persistent) {
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
  TORCH_CHECK(unroll == 0 || unroll == 4 || unroll == 8 || unroll == 16 ||
                  unroll == 32,
              "unroll must be 0 (auto), 4, 8, or 16 or 32 (stream kernel)");
  const int tiles = (N + 15) / 16;
  auto stream = c10::hip::getCurrentHIPStream();
  if (skinny_use_persistent(persistent, tiles_per_wg != 0 || unroll != 0, M,
                            N, K, tiles, false)) {
    // one variant: a team takes one tile per trip and keeps two groups
    // of KUNROLL chunks in flight (8 per group spills at 1024 threads)
    TORCH_CHECK(tiles_per_wg == 0 && unroll == 0,
                "persistent=1 has no tiles_per_wg or unroll variants");
    PERSIST_LAUNCH(KUNROLL, false, tiles, 16);
    HIP_CHECK_LAST();
    return;
  }
  int snt = 1;
  if (const int chunks = skinny_stream_chunks(unroll, tiles_per_wg, M, N, K,
                                              tiles, x.stride(0), &snt)) {
    const int nt = snt;
    const int grid = (tiles + nt - 1) / nt;
    if (chunks == 32) STREAM_LAUNCH(4, 1, grid, 16);
    else if (nt == 2) STREAM_LAUNCH(2, 2, grid, 32);
    else STREAM_LAUNCH(2, 1, grid, 16);
    HIP_CHECK_LAST();
    return;
  }
  const int nt =
      tiles_per_wg ? (int)tiles_per_wg : skinny_auto_tiles(M, tiles);
  const int grid = (tiles + nt - 1) / nt;
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
                             torch::Tensor w, int64_t persistent) {
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
  if (skinny_use_persistent(persistent, false, M, N, K, grid, true)) {
    PERSIST_LAUNCH(KUNROLL, true, grid, I);
    HIP_CHECK_LAST();
    return;
  }
  if (skinny_unroll(K, 0) == 8)
    SKINNY_LAUNCH(8, 2, true, grid, 16, I);
  else
    SKINNY_LAUNCH(4, 2, true, grid, 16, I);
  HIP_CHECK_LAST();
}
#undef SKINNY_LAUNCH
#undef STREAM_LAUNCH
#undef PERSIST_LAUNCH
