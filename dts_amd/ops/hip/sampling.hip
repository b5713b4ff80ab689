// Fused temperature-softmax + nucleus (top-p) sampling for MI355X.
//
// Sort-free, histogram-thresholded design: instead of sorting 128k logits
// per row (the classic CUDA approach) or bisecting a threshold with ~24
// full passes, one pass builds a 1024-bin LDS histogram of the softmax
// masses over y = (logit - max)/T ∈ [-30, 0]; a suffix scan of the bins
// picks the threshold bin whose cumulative mass reaches top_p, and one
// final pass draws the token from the kept set via a two-level prefix
// walk. 3 full passes total (max; histogram+Z; select) — each streams the
// row out of L2 (a 128k-fp32 row is 512 KB ≪ the 4 MiB per-XCD L2).
//
// The kept-mass overshoot from taking a whole boundary bin is ≤ the bin
// mass (bin width 0.03 in y), i.e. the cut differs from an exact top-p by
// at most a handful of borderline tokens — the same class of tie-handling
// slack that sorting implementations have at equal probabilities.
//
// Each row is one 256-thread workgroup; thread t owns the STRIDED element
// set {t, t+256, ...} in every pass — contiguous per-thread ranges made
// every lane touch a different cache line per 4-byte read (measured 16x
// bandwidth waste, ~436 us/row). The final draw walks the owner thread's
// strided set in stride-order: a fixed permutation of the kept set, which
// leaves each token's selection probability unchanged. RNG: per-row
// xorshift from a seed (deterministic given seed).
//
// Semantics match dts_amd/ops/torch_ref.py top_p_sample (temperature<=0
// => greedy; at-least-one-token guarantee).

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#define NBINS 1024
#define YMIN (-30.0f)

DEV unsigned long long xorshift64(unsigned long long x) {
  x ^= x << 13;
  x ^= x >> 7;
  x ^= x << 17;
  return x;
}

// splitmix64-style stateless seed mix over (base, position): the SAME
// formula runs on the host (dts_amd/ops/torch_ref.py mix_seed) so the
// chained-decode path (seeds derived on device from static positions)
// draws the exact token the per-step host path would.
DEV unsigned long long mix_seed64(unsigned long long base,
                                  unsigned long long pos) {
  unsigned long long x = base ^ (pos * 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x & 0x7FFFFFFFull;
}

// out[i] = mix(base[i], positions[i] + 1): positions are QUERY positions
// of the decode rows; the drawn token's index is one past the query.
__global__ void derive_seeds_kernel(long* __restrict__ out,
                                    const long* __restrict__ bases,
                                    const long* __restrict__ positions,
                                    int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = (long)mix_seed64((unsigned long long)bases[i],
                              (unsigned long long)(positions[i] + 1));
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
top_p_sample_kernel(long* __restrict__ out, const float* __restrict__ logits,
                    const float* __restrict__ temps,
                    const float* __restrict__ top_ps,
                    const long* __restrict__ seeds, int V) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const float* x = logits + (long)row * V;
  const float T = temps[row];
  const float p_target = top_ps[row];

  __shared__ float red[BLOCK / WAVE];
  __shared__ float s_bcast[2];
  __shared__ int s_argmax;
  __shared__ float s_bins[NBINS];

  // ---- pass 1: max (and argmax for greedy)
  float mymax = -1e30f;
  int myarg = 0;
  for (int i = tid; i < V; i += BLOCK) {
    float v = x[i];
    if (v > mymax) {
      mymax = v;
      myarg = i;
    }
  }
  {
    float wm = mymax;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      wm = fmaxf(wm, __shfl_xor(wm, off, 64));
    if ((tid & 63) == 0) red[tid / 64] = wm;
    __syncthreads();
    float bm = -1e30f;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) bm = fmaxf(bm, red[i]);
    if (T <= 0.f) {
      // deterministic tie-break: LOWEST index among equal maxima (the
      // torch reference argmax does the same; an atomicCAS race here
      // made chained-vs-stepped greedy streams diverge on real ties)
      if (tid == 0) s_argmax = 0x7FFFFFFF;
      __syncthreads();
      if (mymax == bm) atomicMin(&s_argmax, myarg);
      __syncthreads();
      if (tid == 0) out[row] = s_argmax;
      return;
    }
    if (tid == 0) s_bcast[0] = bm;
    __syncthreads();
  }
  const float m = s_bcast[0];
  const float invT = 1.f / T;

  // ---- pass 2: mass histogram over y + total Z
  for (int b = tid; b < NBINS; b += BLOCK) s_bins[b] = 0.f;
  __syncthreads();
  float zpart = 0.f;
  const float bin_scale = NBINS / (-YMIN);  // bins per unit y
  for (int i = tid; i < V; i += BLOCK) {
    float y = (x[i] - m) * invT;
    float e = __expf(y);
    zpart += e;
    if (y > YMIN) {
      int b = (int)fminf((y - YMIN) * bin_scale, (float)(NBINS - 1));
      atomicAdd(&s_bins[b], e);
    }
  }
  {
    float z = wave_sum(zpart);
    if ((tid & 63) == 0) red[tid / 64] = z;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) tot += red[i];
    if (tid == 0) s_bcast[1] = tot;
    __syncthreads();
  }
  const float Z = s_bcast[1];

  // ---- threshold: suffix-scan the bins from the top until >= p*Z
  // (serial over 1024 bins on thread 0 — trivial vs a vocab pass)
  if (tid == 0) {
    const float target = fminf(p_target, 1.0f) * Z;
    float acc = 0.f;
    int b = NBINS - 1;
    for (; b >= 0; --b) {
      acc += s_bins[b];
      if (acc >= target) break;
    }
    if (b < 0) b = 0;
    s_bcast[0] = YMIN + b / bin_scale;  // tau = lower edge of boundary bin
  }
  __syncthreads();
  const float tau = s_bcast[0];

  // ---- kept mass per thread + prefix over threads
  __shared__ float s_pref[BLOCK + 1];
  float mymass = 0.f;
  for (int i = tid; i < V; i += BLOCK) {
    float y = (x[i] - m) * invT;
    if (y >= tau) mymass += __expf(y);
  }
  s_pref[tid + 1] = mymass;
  __syncthreads();
  if (tid == 0) {
    s_pref[0] = 0.f;
    for (int i = 1; i <= BLOCK; ++i) s_pref[i] += s_pref[i - 1];
  }
  __syncthreads();
  const float total_kept = s_pref[BLOCK];

  // ---- draw u and locate the owning thread/token
  unsigned long long rng =
      xorshift64((unsigned long long)seeds[row] * 2685821657736338717ULL + 1);
  rng = xorshift64(rng);
  const float u =
      (float)((rng >> 11) * (1.0 / 9007199254740992.0)) * total_kept;

  __shared__ long s_result;
  if (tid == 0) s_result = -1;
  __syncthreads();
  if (total_kept > 0.f && u >= s_pref[tid] && u < s_pref[tid + 1]) {
    float acc = s_pref[tid];
    long pick = -1, last_kept = -1;
    for (int i = tid; i < V; i += BLOCK) {
      float y = (x[i] - m) * invT;
      if (y >= tau) {
        last_kept = i;
        acc += __expf(y);
        if (acc > u) {
          pick = i;
          break;
        }
      }
    }
    s_result = (pick >= 0) ? pick : last_kept;
  }
  __syncthreads();
  if (tid == 0) {
    long r = s_result;
    if (r < 0) {
      // degenerate: nothing kept — greedy fallback via serial scan
      float bm = -1e30f;
      for (int i = 0; i < V; ++i)
        if (x[i] > bm) {
          bm = x[i];
          r = i;
        }
    }
    out[row] = r;
  }
}

// ---------------------------------------------------------------------------
// Gridded sampler (v2): the one-workgroup-per-row design above leaves
// 250 of 256 CUs idle at decode batch widths (B=1..8) — measured 364 us
// avg on the r2 bench (4.9% of GPU busy). v2 splits each row's vocab
// across SLICES workgroups and runs five tiny gridded kernels:
//   s2_max   : per-slice max -> packed 64-bit atomicMax (value bits
//              high, ~index low => deterministic LOWEST-index tie-break)
//   s2_hist  : per-slice LDS histogram of exp masses over
//              y=(x-max)/T in [-30,0] -> atomicAdd into global bins
//   s2_tau   : per-row 1024-bin suffix scan -> threshold tau
//   s2_kept  : per-slice EXACT kept mass (y >= tau)
//   s2_draw  : per-row: prefix over slice masses, draw u, walk the one
//              owning slice with a two-level prefix to pick the token
// Same bins / y-space / boundary-bin slack as v1; the draw walks in
// slice-index order (a different fixed permutation of the kept set than
// v1's strided order — same distribution, different exact picks for a
// given seed). Greedy (T<=0) short-circuits after s2_max.
// ---------------------------------------------------------------------------

#define S2_SLICES 16

DEV unsigned long long pack_max(float v, int idx) {
  union { float f; unsigned int i; } c;
  c.f = v;
  // order-preserving float->uint (sign flip trick)
  unsigned int bits = (c.i & 0x80000000u) ? ~c.i : (c.i | 0x80000000u);
  return ((unsigned long long)bits << 32) | (unsigned int)(0x7FFFFFFF - idx);
}

__global__ void __launch_bounds__(256)
s2_max_kernel(unsigned long long* __restrict__ gmax,
              const float* __restrict__ logits, int V) {
  const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  float m = -1e30f;
  int arg = lo;
  for (int i = lo + tid; i < hi; i += 256) {
    if (x[i] > m) { m = x[i]; arg = i; }
  }
  // wave+wg reduce via LDS on packed values (max keeps lowest index)
  __shared__ unsigned long long red[4];
  unsigned long long p = pack_max(m, arg);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_xor((long long)p, off, 64);
    if (o > p) p = o;
  }
  if ((tid & 63) == 0) red[tid / 64] = p;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i) if (red[i] > p) p = red[i];
    atomicMax(gmax + row, p);
  }
}

__global__ void __launch_bounds__(256)
s2_hist_kernel(float* __restrict__ gbins,  // [S, NBINS]
               const unsigned long long* __restrict__ gmax,
               const float* __restrict__ logits,
               const float* __restrict__ temps, int V) {
  const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float T = temps[row];
  if (T <= 0.f) return;  // greedy: resolved from gmax alone
  union { unsigned int i; float f; } c;
  unsigned int bits = (unsigned int)(gmax[row] >> 32);
  c.i = (bits & 0x80000000u) ? (bits & 0x7FFFFFFFu) : ~bits;
  const float m = c.f;
  const float invT = 1.f / T;
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  __shared__ float s_bins[NBINS];
  for (int b = tid; b < NBINS; b += 256) s_bins[b] = 0.f;
  __syncthreads();
  const float bin_scale = NBINS / (-YMIN);
  for (int i = lo + tid; i < hi; i += 256) {
    float y = (x[i] - m) * invT;
    if (y > YMIN) {
      int b = (int)fminf((y - YMIN) * bin_scale, (float)(NBINS - 1));
      atomicAdd(&s_bins[b], __expf(y));
    }
  }
  __syncthreads();
  float* dst = gbins + (long)row * NBINS;
  for (int b = tid; b < NBINS; b += 256)
    if (s_bins[b] != 0.f) atomicAdd(dst + b, s_bins[b]);
}

__global__ void __launch_bounds__(256)
s2_tau_kernel(float* __restrict__ gtau, long* __restrict__ out,
              const float* __restrict__ gbins,
              const unsigned long long* __restrict__ gmax,
              const float* __restrict__ temps,
              const float* __restrict__ top_ps) {
  const int row = blockIdx.x;
  if (temps[row] <= 0.f) {
    if (threadIdx.x == 0)
      out[row] = 0x7FFFFFFF - (int)(gmax[row] & 0xFFFFFFFFull);
    return;
  }
  if (threadIdx.x != 0) return;
  const float* bins = gbins + (long)row * NBINS;
  float Z = 0.f;
  for (int b = 0; b < NBINS; ++b) Z += bins[b];
  const float target = fminf(top_ps[row], 1.0f) * Z;
  float acc = 0.f;
  int b = NBINS - 1;
  for (; b >= 0; --b) {
    acc += bins[b];
    if (acc >= target) break;
  }
  if (b < 0) b = 0;
  gtau[row] = YMIN + b * (-YMIN) / NBINS;
}

__global__ void __launch_bounds__(256)
s2_kept_kernel(float* __restrict__ gslice,  // [S, S2_SLICES]
               const float* __restrict__ gtau,
               const unsigned long long* __restrict__ gmax,
               const float* __restrict__ logits,
               const float* __restrict__ temps, int V) {
  const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float T = temps[row];
  if (T <= 0.f) return;
  union { unsigned int i; float f; } c;
  unsigned int bits = (unsigned int)(gmax[row] >> 32);
  c.i = (bits & 0x80000000u) ? (bits & 0x7FFFFFFFu) : ~bits;
  const float m = c.f;
  const float invT = 1.f / T, tau = gtau[row];
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  float mass = 0.f;
  for (int i = lo + tid; i < hi; i += 256) {
    float y = (x[i] - m) * invT;
    if (y >= tau) mass += __expf(y);
  }
  mass = wave_sum(mass);
  __shared__ float red[4];
  if ((tid & 63) == 0) red[tid / 64] = mass;
  __syncthreads();
  if (tid == 0)
    gslice[(long)row * S2_SLICES + slice] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256)
s2_draw_kernel(long* __restrict__ out, const float* __restrict__ gslice,
               const float* __restrict__ gtau,
               const unsigned long long* __restrict__ gmax,
               const float* __restrict__ logits,
               const float* __restrict__ temps,
               const long* __restrict__ seeds, int V) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float T = temps[row];
  if (T <= 0.f) return;  // already written by s2_tau
  union { unsigned int i; float f; } c;
  unsigned int bits = (unsigned int)(gmax[row] >> 32);
  c.i = (bits & 0x80000000u) ? (bits & 0x7FFFFFFFu) : ~bits;
  const float m = c.f;
  const float invT = 1.f / T, tau = gtau[row];
  const float* sl = gslice + (long)row * S2_SLICES;
  __shared__ float s_pref_sl[S2_SLICES + 1];
  __shared__ int s_slice;
  __shared__ float s_u;
  if (tid == 0) {
    s_pref_sl[0] = 0.f;
    for (int i = 0; i < S2_SLICES; ++i) s_pref_sl[i + 1] = s_pref_sl[i] + sl[i];
    const float total = s_pref_sl[S2_SLICES];
    unsigned long long rng =
        xorshift64((unsigned long long)seeds[row] * 2685821657736338717ULL + 1);
    rng = xorshift64(rng);
    float u = (float)((rng >> 11) * (1.0 / 9007199254740992.0)) * total;
    int s = 0;
    while (s < S2_SLICES - 1 && u >= s_pref_sl[s + 1]) ++s;
    s_slice = s;
    s_u = u - s_pref_sl[s];
  }
  __syncthreads();
  const int slice = s_slice;
  const float u = s_u;
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  // two-level prefix inside the slice: thread t owns [lo + t*chunk ...)
  const int n = hi - lo;
  const int chunk = (n + 255) / 256;
  const int my_lo = lo + tid * chunk;
  const int my_hi = min(hi, my_lo + chunk);
  float mymass = 0.f;
  for (int i = my_lo; i < my_hi; ++i) {
    float y = (x[i] - m) * invT;
    if (y >= tau) mymass += __expf(y);
  }
  __shared__ float s_pref[257];
  s_pref[tid + 1] = mymass;
  __syncthreads();
  if (tid == 0) {
    s_pref[0] = 0.f;
    for (int i = 1; i <= 256; ++i) s_pref[i] += s_pref[i - 1];
  }
  __syncthreads();
  __shared__ long s_result;
  if (tid == 0) s_result = -1;
  __syncthreads();
  if (u >= s_pref[tid] && u < s_pref[tid + 1]) {
    float acc = s_pref[tid];
    long pick = -1, last_kept = -1;
    for (int i = my_lo; i < my_hi; ++i) {
      float y = (x[i] - m) * invT;
      if (y >= tau) {
        last_kept = i;
        acc += __expf(y);
        if (acc > u) { pick = i; break; }
      }
    }
    s_result = (pick >= 0) ? pick : last_kept;
  }
  __syncthreads();
  if (tid == 0) {
    long r = s_result;
    if (r < 0) {
      // degenerate (fp slack at the edge): greedy fallback from gmax
      r = 0x7FFFFFFF - (int)(gmax[row] & 0xFFFFFFFFull);
    }
    out[row] = r;
  }
}

void top_p_sample_v2(torch::Tensor out, torch::Tensor logits,
                     torch::Tensor temps, torch::Tensor top_ps,
                     torch::Tensor seeds, torch::Tensor ws_max,
                     torch::Tensor ws_bins, torch::Tensor ws_slice,
                     torch::Tensor ws_tau) {
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32 && logits.is_contiguous());
  const int S = logits.size(0), V = logits.size(1);
  auto stream = c10::hip::getCurrentHIPStream();
  hipMemsetAsync(ws_max.data_ptr(), 0, S * 8, stream);
  hipMemsetAsync(ws_bins.data_ptr(), 0, (long)S * NBINS * 4, stream);
  dim3 gs(S, S2_SLICES);
  hipLaunchKernelGGL(s2_max_kernel, gs, dim3(256), 0, stream,
                     (unsigned long long*)ws_max.data_ptr(),
                     (const float*)logits.data_ptr(), V);
  hipLaunchKernelGGL(s2_hist_kernel, gs, dim3(256), 0, stream,
                     (float*)ws_bins.data_ptr(),
                     (const unsigned long long*)ws_max.data_ptr(),
                     (const float*)logits.data_ptr(),
                     (const float*)temps.data_ptr(), V);
  hipLaunchKernelGGL(s2_tau_kernel, dim3(S), dim3(256), 0, stream,
                     (float*)ws_tau.data_ptr(), (long*)out.data_ptr(),
                     (const float*)ws_bins.data_ptr(),
                     (const unsigned long long*)ws_max.data_ptr(),
                     (const float*)temps.data_ptr(),
                     (const float*)top_ps.data_ptr());
  hipLaunchKernelGGL(s2_kept_kernel, gs, dim3(256), 0, stream,
                     (float*)ws_slice.data_ptr(),
                     (const float*)ws_tau.data_ptr(),
                     (const unsigned long long*)ws_max.data_ptr(),
                     (const float*)logits.data_ptr(),
                     (const float*)temps.data_ptr(), V);
  hipLaunchKernelGGL(s2_draw_kernel, dim3(S), dim3(256), 0, stream,
                     (long*)out.data_ptr(), (const float*)ws_slice.data_ptr(),
                     (const float*)ws_tau.data_ptr(),
                     (const unsigned long long*)ws_max.data_ptr(),
                     (const float*)logits.data_ptr(),
                     (const float*)temps.data_ptr(),
                     (const long*)seeds.data_ptr(), V);
  HIP_CHECK_LAST();
}

void derive_seeds(torch::Tensor out, torch::Tensor bases,
                  torch::Tensor positions) {
  const int n = out.size(0);
  hipLaunchKernelGGL(derive_seeds_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     c10::hip::getCurrentHIPStream(), (long*)out.data_ptr(),
                     (const long*)bases.data_ptr(),
                     (const long*)positions.data_ptr(), n);
  HIP_CHECK_LAST();
}

void top_p_sample(torch::Tensor out, torch::Tensor logits, torch::Tensor temps,
                  torch::Tensor top_ps, torch::Tensor seeds) {
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32 && logits.is_contiguous());
  const int S = logits.size(0), V = logits.size(1);
  hipLaunchKernelGGL((top_p_sample_kernel<256>), dim3(S), dim3(256), 0,
                     c10::hip::getCurrentHIPStream(), (long*)out.data_ptr(),
                     (const float*)logits.data_ptr(),
                     (const float*)temps.data_ptr(),
                     (const float*)top_ps.data_ptr(),
                     (const long*)seeds.data_ptr(), V);
  HIP_CHECK_LAST();
}

// ---------------------------------------------------------------------------
// top-k / min-p filtered sampling (sample_filtered, sample_filtered_v2).
//
// Order, as dts_amd/ops/torch_ref.py defines it: top-k, then top-p over
// the distribution renormalised to the top-k survivors, then min-p, then
// the draw. The unfiltered kernels above are not touched: a request with
// top_k == 0 and min_p == 0 never reaches this half of the file, and a
// disabled row inside a filtered call runs the same arithmetic as above
// (xk = -inf, tau = tau_p).
//
// top-k: exact k-th largest logit by a radix select over the
// order-preserving float->uint32 key of pack_max, 11/11/10 bits from the
// top, no sort. Counts are integers (ds_add_u32 in LDS, unsigned atomicAdd
// into a per-row global array), so the k-th key is exact and independent
// of scheduling. Membership is x[i] >= xk on the LOGIT, ties included:
// y = (x - m) * invT is monotone but not injective in fp32, so y >= y_k
// would let in tokens that are neither in the top k nor tied with the
// k-th. The kept-mass and draw walks test x[i] >= xk && y >= tau.
//
// Gridded form: one count kernel per pass on v2's (S, 16 slices) grid.
// Every workgroup re-derives the digits chosen so far from the global
// counts of the earlier passes in its prologue (<= 3 scans of <= 2048
// bins), so no one-workgroup kernel sits between the passes. Rows with
// top-k disabled (k < 1 or k >= V) or T <= 0 leave the count kernels at
// once.
//
// min-p: p_i / p_max = exp(y_i), so the cut is y_i >= logf(min_p); it
// folds into tau = max(tau_p, logf(min_p)) and needs no pass of its own.
//
// Unchanged from the kernels above: a token with y <= -30 is never drawn
// (tau >= YMIN), inside the top-k set or not; and v1, v2 and the CPU
// reference draw different tokens for one seed (different walk orders, a
// different RNG on the CPU) -- they share the kept set and the
// distribution, not the draws.
// ---------------------------------------------------------------------------

#define SEL_PASSES 3
#define SEL_BINS 2048  // bins of the widest pass (11 bits)

DEV unsigned int sel_key(float v) {
  union { float f; unsigned int i; } c;
  c.f = v;
  return (c.i & 0x80000000u) ? ~c.i : (c.i | 0x80000000u);
}

DEV float sel_unkey(unsigned int bits) {
  union { unsigned int i; float f; } c;
  c.i = (bits & 0x80000000u) ? (bits & 0x7FFFFFFFu) : ~bits;
  return c.f;
}

DEV int sel_bits(int pass) { return pass == 2 ? 10 : 11; }
DEV int sel_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }

// All 256 threads of the workgroup. cnt[0..nb) are the counts of one
// digit (nb = 1024 or 2048; LDS or global). Finds the digit d with
//   sum(cnt[d+1..nb)) < krem <= sum(cnt[d..nb))
// i.e. the digit of the krem-th largest key, and the rank that remains
// inside that digit. Thread t owns bins [t*per, (t+1)*per).
DEV void select_digit(const unsigned int* cnt, int nb, unsigned int& krem,
                      unsigned int& digit, unsigned int* s_wave,
                      unsigned int* s_out) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int per = nb >> 8;  // 4 or 8
  unsigned int c[8];
  unsigned int mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = (j < per) ? cnt[tid * per + j] : 0u;
    mine += c[j];
  }
  unsigned int suf = mine;  // inclusive suffix sum within the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned int o = __shfl_down(suf, off, 64);
    if (lane + off < 64) suf += o;
  }
  if (lane == 0) s_wave[tid >> 6] = suf;
  if (tid == 0) {
    s_out[0] = 0;  // only if krem exceeds the total, which k < V excludes
    s_out[1] = 1;
  }
  __syncthreads();
  unsigned int above = suf - mine;
  for (int w = (tid >> 6) + 1; w < 4; ++w) above += s_wave[w];
  if (above < krem && krem <= above + mine) {
    bool found = false;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
      if (j < per && !found) {
        if (krem <= above + c[j]) {
          s_out[0] = tid * per + j;
          s_out[1] = krem - above;
          found = true;
        } else {
          above += c[j];
        }
      }
    }
  }
  __syncthreads();
  digit = s_out[0];
  krem = s_out[1];
  __syncthreads();  // s_wave / s_out are reused by the next call
}

// Key bits fixed by the first npass passes of a row's global counts.
DEV void select_prefix(const unsigned int* rowcnt, int npass, unsigned int k,
                       unsigned int& prefix, unsigned int* s_wave,
                       unsigned int* s_out) {
  unsigned int krem = k;
  prefix = 0;
  for (int p = 0; p < npass; ++p) {
    unsigned int d;
    select_digit(rowcnt + p * SEL_BINS, 1 << sel_bits(p), krem, d, s_wave,
                 s_out);
    prefix = (prefix << sel_bits(p)) | d;
  }
}

// One radix-select pass: count digit `pass` of the keys that match the
// digits chosen so far.
__global__ void __launch_bounds__(256)
s2f_count_kernel(unsigned int* __restrict__ gcnt,  // [S, SEL_PASSES, SEL_BINS]
                 const float* __restrict__ logits,
                 const float* __restrict__ temps,
                 const int* __restrict__ top_ks, int V, int pass) {
  const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const int k = top_ks[row];
  if (temps[row] <= 0.f || k < 1 || k >= V) return;
  __shared__ unsigned int s_cnt[SEL_BINS];
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned int s_out[2];
  unsigned int* rowcnt = gcnt + (long)row * SEL_PASSES * SEL_BINS;
  unsigned int prefix;
  select_prefix(rowcnt, pass, (unsigned int)k, prefix, s_wave, s_out);
  const int bits = sel_bits(pass), shift = sel_shift(pass);
  const int nb = 1 << bits;
  for (int b = tid; b < nb; b += 256) s_cnt[b] = 0u;
  __syncthreads();
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  for (int i = lo + tid; i < hi; i += 256) {
    const unsigned int key = sel_key(x[i]);
    if (pass == 0 || (key >> (shift + bits)) == prefix)
      atomicAdd(&s_cnt[(key >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  unsigned int* dst = rowcnt + pass * SEL_BINS;
  for (int b = tid; b < nb; b += 256)
    if (s_cnt[b] != 0u) atomicAdd(dst + b, s_cnt[b]);
}

// s2_hist over the top-k survivors; also resolves xk from the three count
// passes and leaves it in gxk for the kept / draw kernels.
__global__ void __launch_bounds__(256)
s2f_hist_kernel(float* __restrict__ gbins,  // [S, NBINS]
                float* __restrict__ gxk,    // [S]
                const unsigned int* __restrict__ gcnt,
                const unsigned long long* __restrict__ gmax,
                const float* __restrict__ logits,
                const float* __restrict__ temps,
                const int* __restrict__ top_ks, int V) {
  const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float T = temps[row];
  if (T <= 0.f) return;  // greedy: resolved from gmax alone
  __shared__ float s_bins[NBINS];
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned int s_out[2];
  float xk = -INFINITY;
  const int k = top_ks[row];
  if (k >= 1 && k < V) {
    unsigned int prefix;
    select_prefix(gcnt + (long)row * SEL_PASSES * SEL_BINS, SEL_PASSES,
                  (unsigned int)k, prefix, s_wave, s_out);
    xk = sel_unkey(prefix);
  }
  if (slice == 0 && tid == 0) gxk[row] = xk;
  const float m = sel_unkey((unsigned int)(gmax[row] >> 32));
  const float invT = 1.f / T;
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  for (int b = tid; b < NBINS; b += 256) s_bins[b] = 0.f;
  __syncthreads();
  const float bin_scale = NBINS / (-YMIN);
  for (int i = lo + tid; i < hi; i += 256) {
    const float v = x[i];
    if (v < xk) continue;
    float y = (v - m) * invT;
    if (y > YMIN) {
      int b = (int)fminf((y - YMIN) * bin_scale, (float)(NBINS - 1));
      atomicAdd(&s_bins[b], __expf(y));
    }
  }
  __syncthreads();
  float* dst = gbins + (long)row * NBINS;
  for (int b = tid; b < NBINS; b += 256)
    if (s_bins[b] != 0.f) atomicAdd(dst + b, s_bins[b]);
}

// s2_tau with tau = max(tau_p, logf(min_p)); the bins hold the top-k
// survivors only, so the target is top_p * Z_k.
__global__ void __launch_bounds__(256)
s2f_tau_kernel(float* __restrict__ gtau, long* __restrict__ out,
               const float* __restrict__ gbins,
               const unsigned long long* __restrict__ gmax,
               const float* __restrict__ temps,
               const float* __restrict__ top_ps,
               const float* __restrict__ min_ps) {
  const int row = blockIdx.x;
  if (temps[row] <= 0.f) {
    if (threadIdx.x == 0)
      out[row] = 0x7FFFFFFF - (int)(gmax[row] & 0xFFFFFFFFull);
    return;
  }
  if (threadIdx.x != 0) return;
  const float* bins = gbins + (long)row * NBINS;
  float Z = 0.f;
  for (int b = 0; b < NBINS; ++b) Z += bins[b];
  const float target = fminf(top_ps[row], 1.0f) * Z;
  float acc = 0.f;
  int b = NBINS - 1;
  for (; b >= 0; --b) {
    acc += bins[b];
    if (acc >= target) break;
  }
  if (b < 0) b = 0;
  float tau = YMIN + b * (-YMIN) / NBINS;
  const float mp = min_ps[row];
  if (mp > 0.f) tau = fmaxf(tau, logf(mp));
  gtau[row] = tau;
}

__global__ void __launch_bounds__(256)
s2f_kept_kernel(float* __restrict__ gslice,  // [S, S2_SLICES]
                const float* __restrict__ gtau,
                const float* __restrict__ gxk,
                const unsigned long long* __restrict__ gmax,
                const float* __restrict__ logits,
                const float* __restrict__ temps, int V) {
  const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float T = temps[row];
  if (T <= 0.f) return;
  const float m = sel_unkey((unsigned int)(gmax[row] >> 32));
  const float invT = 1.f / T, tau = gtau[row], xk = gxk[row];
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  float mass = 0.f;
  for (int i = lo + tid; i < hi; i += 256) {
    const float v = x[i];
    float y = (v - m) * invT;
    if (v >= xk && y >= tau) mass += __expf(y);
  }
  mass = wave_sum(mass);
  __shared__ float red[4];
  if ((tid & 63) == 0) red[tid / 64] = mass;
  __syncthreads();
  if (tid == 0)
    gslice[(long)row * S2_SLICES + slice] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256)
s2f_draw_kernel(long* __restrict__ out, const float* __restrict__ gslice,
                const float* __restrict__ gtau, const float* __restrict__ gxk,
                const unsigned long long* __restrict__ gmax,
                const float* __restrict__ logits,
                const float* __restrict__ temps,
                const long* __restrict__ seeds, int V) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float T = temps[row];
  if (T <= 0.f) return;  // already written by s2f_tau
  const float m = sel_unkey((unsigned int)(gmax[row] >> 32));
  const float invT = 1.f / T, tau = gtau[row], xk = gxk[row];
  const float* sl = gslice + (long)row * S2_SLICES;
  __shared__ float s_pref_sl[S2_SLICES + 1];
  __shared__ int s_slice;
  __shared__ float s_u;
  if (tid == 0) {
    s_pref_sl[0] = 0.f;
    for (int i = 0; i < S2_SLICES; ++i) s_pref_sl[i + 1] = s_pref_sl[i] + sl[i];
    const float total = s_pref_sl[S2_SLICES];
    unsigned long long rng =
        xorshift64((unsigned long long)seeds[row] * 2685821657736338717ULL + 1);
    rng = xorshift64(rng);
    float u = (float)((rng >> 11) * (1.0 / 9007199254740992.0)) * total;
    int s = 0;
    while (s < S2_SLICES - 1 && u >= s_pref_sl[s + 1]) ++s;
    s_slice = s;
    s_u = u - s_pref_sl[s];
  }
  __syncthreads();
  const int slice = s_slice;
  const float u = s_u;
  const float* x = logits + (long)row * V;
  const int lo = slice * V / S2_SLICES, hi = (slice + 1) * V / S2_SLICES;
  const int n = hi - lo;
  const int chunk = (n + 255) / 256;
  const int my_lo = lo + tid * chunk;
  const int my_hi = min(hi, my_lo + chunk);
  float mymass = 0.f;
  for (int i = my_lo; i < my_hi; ++i) {
    const float v = x[i];
    float y = (v - m) * invT;
    if (v >= xk && y >= tau) mymass += __expf(y);
  }
  __shared__ float s_pref[257];
  s_pref[tid + 1] = mymass;
  __syncthreads();
  if (tid == 0) {
    s_pref[0] = 0.f;
    for (int i = 1; i <= 256; ++i) s_pref[i] += s_pref[i - 1];
  }
  __syncthreads();
  __shared__ long s_result;
  if (tid == 0) s_result = -1;
  __syncthreads();
  if (u >= s_pref[tid] && u < s_pref[tid + 1]) {
    float acc = s_pref[tid];
    long pick = -1, last_kept = -1;
    for (int i = my_lo; i < my_hi; ++i) {
      const float v = x[i];
      float y = (v - m) * invT;
      if (v >= xk && y >= tau) {
        last_kept = i;
        acc += __expf(y);
        if (acc > u) { pick = i; break; }
      }
    }
    s_result = (pick >= 0) ? pick : last_kept;
  }
  __syncthreads();
  if (tid == 0) {
    long r = s_result;
    if (r < 0) {
      // degenerate (fp slack at the edge): greedy fallback from gmax
      r = 0x7FFFFFFF - (int)(gmax[row] & 0xFFFFFFFFull);
    }
    out[row] = r;
  }
}

// One workgroup per row (v1 layout): the select runs in LDS between the
// max pass and the histogram.
__global__ void __launch_bounds__(256)
sample_filtered_kernel(long* __restrict__ out,
                       const float* __restrict__ logits,
                       const float* __restrict__ temps,
                       const float* __restrict__ top_ps,
                       const int* __restrict__ top_ks,
                       const float* __restrict__ min_ps,
                       const long* __restrict__ seeds, int V) {
  constexpr int BLOCK = 256;
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const float* x = logits + (long)row * V;
  const float T = temps[row];
  const float p_target = top_ps[row];

  __shared__ float red[BLOCK / WAVE];
  __shared__ float s_bcast[2];
  __shared__ int s_argmax;
  __shared__ float s_bins[NBINS];
  __shared__ unsigned int s_cnt[SEL_BINS];
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned int s_out[2];

  // ---- pass 1: max (and argmax for greedy)
  float mymax = -1e30f;
  int myarg = 0;
  for (int i = tid; i < V; i += BLOCK) {
    float v = x[i];
    if (v > mymax) {
      mymax = v;
      myarg = i;
    }
  }
  {
    float wm = mymax;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      wm = fmaxf(wm, __shfl_xor(wm, off, 64));
    if ((tid & 63) == 0) red[tid / 64] = wm;
    __syncthreads();
    float bm = -1e30f;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) bm = fmaxf(bm, red[i]);
    if (T <= 0.f) {
      if (tid == 0) s_argmax = 0x7FFFFFFF;
      __syncthreads();
      if (mymax == bm) atomicMin(&s_argmax, myarg);
      __syncthreads();
      if (tid == 0) out[row] = s_argmax;
      return;
    }
    if (tid == 0) s_bcast[0] = bm;
    __syncthreads();
  }
  const float m = s_bcast[0];
  const float invT = 1.f / T;

  // ---- top-k: radix select of the k-th largest logit
  float xk = -INFINITY;
  const int k = top_ks[row];
  if (k >= 1 && k < V) {
    unsigned int prefix = 0, krem = (unsigned int)k;
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
      const int bits = sel_bits(pass), shift = sel_shift(pass);
      const int nb = 1 << bits;
      for (int b = tid; b < nb; b += BLOCK) s_cnt[b] = 0u;
      __syncthreads();
      for (int i = tid; i < V; i += BLOCK) {
        const unsigned int key = sel_key(x[i]);
        if (pass == 0 || (key >> (shift + bits)) == prefix)
          atomicAdd(&s_cnt[(key >> shift) & (nb - 1)], 1u);
      }
      __syncthreads();
      unsigned int d;
      select_digit(s_cnt, nb, krem, d, s_wave, s_out);
      prefix = (prefix << bits) | d;
    }
    xk = sel_unkey(prefix);
  }

  // ---- pass 2: mass histogram over y + Z, top-k survivors only
  for (int b = tid; b < NBINS; b += BLOCK) s_bins[b] = 0.f;
  __syncthreads();
  float zpart = 0.f;
  const float bin_scale = NBINS / (-YMIN);  // bins per unit y
  for (int i = tid; i < V; i += BLOCK) {
    const float v = x[i];
    if (v < xk) continue;
    float y = (v - m) * invT;
    float e = __expf(y);
    zpart += e;
    if (y > YMIN) {
      int b = (int)fminf((y - YMIN) * bin_scale, (float)(NBINS - 1));
      atomicAdd(&s_bins[b], e);
    }
  }
  {
    float z = wave_sum(zpart);
    if ((tid & 63) == 0) red[tid / 64] = z;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) tot += red[i];
    if (tid == 0) s_bcast[1] = tot;
    __syncthreads();
  }
  const float Z = s_bcast[1];

  // ---- threshold: tau_p from the suffix scan, then the min-p cut
  if (tid == 0) {
    const float target = fminf(p_target, 1.0f) * Z;
    float acc = 0.f;
    int b = NBINS - 1;
    for (; b >= 0; --b) {
      acc += s_bins[b];
      if (acc >= target) break;
    }
    if (b < 0) b = 0;
    float t = YMIN + b / bin_scale;  // lower edge of the boundary bin
    const float mp = min_ps[row];
    if (mp > 0.f) t = fmaxf(t, logf(mp));
    s_bcast[0] = t;
  }
  __syncthreads();
  const float tau = s_bcast[0];

  // ---- kept mass per thread + prefix over threads
  __shared__ float s_pref[BLOCK + 1];
  float mymass = 0.f;
  for (int i = tid; i < V; i += BLOCK) {
    const float v = x[i];
    float y = (v - m) * invT;
    if (v >= xk && y >= tau) mymass += __expf(y);
  }
  s_pref[tid + 1] = mymass;
  __syncthreads();
  if (tid == 0) {
    s_pref[0] = 0.f;
    for (int i = 1; i <= BLOCK; ++i) s_pref[i] += s_pref[i - 1];
  }
  __syncthreads();
  const float total_kept = s_pref[BLOCK];

  // ---- draw u and locate the owning thread/token
  unsigned long long rng =
      xorshift64((unsigned long long)seeds[row] * 2685821657736338717ULL + 1);
  rng = xorshift64(rng);
  const float u =
      (float)((rng >> 11) * (1.0 / 9007199254740992.0)) * total_kept;

  __shared__ long s_result;
  if (tid == 0) s_result = -1;
  __syncthreads();
  if (total_kept > 0.f && u >= s_pref[tid] && u < s_pref[tid + 1]) {
    float acc = s_pref[tid];
    long pick = -1, last_kept = -1;
    for (int i = tid; i < V; i += BLOCK) {
      const float v = x[i];
      float y = (v - m) * invT;
      if (v >= xk && y >= tau) {
        last_kept = i;
        acc += __expf(y);
        if (acc > u) {
          pick = i;
          break;
        }
      }
    }
    s_result = (pick >= 0) ? pick : last_kept;
  }
  __syncthreads();
  if (tid == 0) {
    long r = s_result;
    if (r < 0) {
      // degenerate: nothing kept — greedy fallback via serial scan
      float bm = -1e30f;
      for (int i = 0; i < V; ++i)
        if (x[i] > bm) {
          bm = x[i];
          r = i;
        }
    }
    out[row] = r;
  }
}

// Argument checks shared by the two filtered entry points: everything a
// kernel reinterprets is pinned here, before anything is enqueued.
static void check_filtered_args(const torch::Tensor& out,
                                const torch::Tensor& logits,
                                const torch::Tensor& temps,
                                const torch::Tensor& top_ps,
                                const torch::Tensor& top_ks,
                                const torch::Tensor& min_ps,
                                const torch::Tensor& seeds) {
  TORCH_CHECK(logits.is_cuda(), "logits must be a device tensor");
  TORCH_CHECK(logits.dim() == 2 && logits.scalar_type() == torch::kFloat32 &&
                  logits.is_contiguous(),
              "logits must be contiguous fp32 [S, V]");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(0) <= 65535,
              "logits [S, V] needs V >= 1 and S <= 65535");
  const int64_t S = logits.size(0);
  auto vec = [&](const torch::Tensor& t, c10::ScalarType dt, const char* name,
                 const char* dtname) {
    TORCH_CHECK(t.is_cuda() && t.device() == logits.device(), name,
                " must be on the logits' device");
    TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dtname);
    TORCH_CHECK(t.dim() == 1 && t.size(0) == S, name, " must have length S = ",
                S);
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  };
  vec(out, torch::kInt64, "out", "int64");
  vec(temps, torch::kFloat32, "temps", "fp32");
  vec(top_ps, torch::kFloat32, "top_ps", "fp32");
  vec(top_ks, torch::kInt32, "top_ks", "int32");
  vec(min_ps, torch::kFloat32, "min_ps", "fp32");
  vec(seeds, torch::kInt64, "seeds", "int64");
}

static void check_workspace(const torch::Tensor& ws,
                            const torch::Tensor& logits, c10::ScalarType dt,
                            int64_t numel, const char* name,
                            const char* dtname) {
  TORCH_CHECK(ws.is_cuda() && ws.device() == logits.device(), name,
              " must be on the logits' device");
  TORCH_CHECK(ws.scalar_type() == dt, name, " must be ", dtname);
  TORCH_CHECK(ws.is_contiguous() && ws.numel() >= numel, name,
              " must be contiguous with at least ", numel, " elements");
}

void sample_filtered(torch::Tensor out, torch::Tensor logits,
                     torch::Tensor temps, torch::Tensor top_ps,
                     torch::Tensor top_ks, torch::Tensor min_ps,
                     torch::Tensor seeds) {
  check_filtered_args(out, logits, temps, top_ps, top_ks, min_ps, seeds);
  const int S = logits.size(0), V = logits.size(1);
  if (S == 0) return;
  hipLaunchKernelGGL(sample_filtered_kernel, dim3(S), dim3(256), 0,
                     c10::hip::getCurrentHIPStream(), (long*)out.data_ptr(),
                     (const float*)logits.data_ptr(),
                     (const float*)temps.data_ptr(),
                     (const float*)top_ps.data_ptr(),
                     (const int*)top_ks.data_ptr(),
                     (const float*)min_ps.data_ptr(),
                     (const long*)seeds.data_ptr(), V);
  HIP_CHECK_LAST();
}

void sample_filtered_v2(torch::Tensor out, torch::Tensor logits,
                        torch::Tensor temps, torch::Tensor top_ps,
                        torch::Tensor top_ks, torch::Tensor min_ps,
                        torch::Tensor seeds, torch::Tensor ws_max,
                        torch::Tensor ws_bins, torch::Tensor ws_slice,
                        torch::Tensor ws_tau, torch::Tensor ws_cnt,
                        torch::Tensor ws_xk) {
  check_filtered_args(out, logits, temps, top_ps, top_ks, min_ps, seeds);
  const int S = logits.size(0), V = logits.size(1);
  check_workspace(ws_max, logits, torch::kInt64, S, "ws_max", "int64");
  check_workspace(ws_bins, logits, torch::kFloat32, (int64_t)S * NBINS,
                  "ws_bins", "fp32");
  check_workspace(ws_slice, logits, torch::kFloat32, (int64_t)S * S2_SLICES,
                  "ws_slice", "fp32");
  check_workspace(ws_tau, logits, torch::kFloat32, S, "ws_tau", "fp32");
  check_workspace(ws_cnt, logits, torch::kInt32,
                  (int64_t)S * SEL_PASSES * SEL_BINS, "ws_cnt", "int32");
  check_workspace(ws_xk, logits, torch::kFloat32, S, "ws_xk", "fp32");
  if (S == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  hipMemsetAsync(ws_max.data_ptr(), 0, S * 8, stream);
  hipMemsetAsync(ws_bins.data_ptr(), 0, (long)S * NBINS * 4, stream);
  hipMemsetAsync(ws_cnt.data_ptr(), 0, (long)S * SEL_PASSES * SEL_BINS * 4,
                 stream);
  const float* lp = (const float*)logits.data_ptr();
  const float* tp = (const float*)temps.data_ptr();
  const int* kp = (const int*)top_ks.data_ptr();
  unsigned long long* gmax = (unsigned long long*)ws_max.data_ptr();
  unsigned int* gcnt = (unsigned int*)ws_cnt.data_ptr();
  dim3 gs(S, S2_SLICES);
  hipLaunchKernelGGL(s2_max_kernel, gs, dim3(256), 0, stream, gmax, lp, V);
  for (int pass = 0; pass < SEL_PASSES; ++pass)
    hipLaunchKernelGGL(s2f_count_kernel, gs, dim3(256), 0, stream, gcnt, lp,
                       tp, kp, V, pass);
  hipLaunchKernelGGL(s2f_hist_kernel, gs, dim3(256), 0, stream,
                     (float*)ws_bins.data_ptr(), (float*)ws_xk.data_ptr(),
                     (const unsigned int*)gcnt,
                     (const unsigned long long*)gmax, lp, tp, kp, V);
  hipLaunchKernelGGL(s2f_tau_kernel, dim3(S), dim3(256), 0, stream,
                     (float*)ws_tau.data_ptr(), (long*)out.data_ptr(),
                     (const float*)ws_bins.data_ptr(),
                     (const unsigned long long*)gmax, tp,
                     (const float*)top_ps.data_ptr(),
                     (const float*)min_ps.data_ptr());
  hipLaunchKernelGGL(s2f_kept_kernel, gs, dim3(256), 0, stream,
                     (float*)ws_slice.data_ptr(),
                     (const float*)ws_tau.data_ptr(),
                     (const float*)ws_xk.data_ptr(),
                     (const unsigned long long*)gmax, lp, tp, V);
  hipLaunchKernelGGL(s2f_draw_kernel, dim3(S), dim3(256), 0, stream,
                     (long*)out.data_ptr(), (const float*)ws_slice.data_ptr(),
                     (const float*)ws_tau.data_ptr(),
                     (const float*)ws_xk.data_ptr(),
                     (const unsigned long long*)gmax, lp, tp,
                     (const long*)seeds.data_ptr(), V);
  HIP_CHECK_LAST();
}
