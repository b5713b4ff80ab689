// MoE routing, expert sort and combine around the grouped GEMMs (gfx950).
//
// Three kernels replace the chain of small torch launches that MoEMLP runs
// per layer around moe_grouped_linear / moe_grouped_gemm. None has a
// workspace, a host sync or an atomic: each is hipGraph-capturable as it
// stands, and each result is a pure function of its inputs.
//
//   moe_route_kernel        one 4-wave workgroup per token. Every wave holds
//             the token's row in registers (lane l owns the 16 B pieces l,
//             l + 64, ...; NCH pieces per lane, a template parameter picked
//             from H; rows past 8192 columns are re-read per expert, they hit
//             L1). Wave w computes the logits of experts w, w + 4, ...: one
//             16 B load of router_w per piece, fp32 accumulation, wave_sum.
//             The E <= 64 logits go through LDS to one lane each of wave 0:
//             softmax over all E, k rounds of wave arg-max (lowest index wins
//             a tie), then w_j = p_j / (p_0 + ... + p_{k-1}), summed in
//             ascending j: the formula and order of softmax -> topk ->
//             renormalise, in fp32.
//   moe_sort_gather_kernel  grid max(P, E), P = T * k assignments. Workgroup
//             p scans the whole experts array (<= 32 KB, L2-resident) once:
//             a ballot and a popcount per wave and 256 elements, so the
//             counts are wave-uniform integers, then four LDS words across
//             the waves. dst[p] = #{q : e_q < e_p} + #{q < p : e_q = e_p} is
//             the row a stable sort by expert gives assignment p; workgroups
//             e < E count counts[e] = #{q : e_q = e} and offsets[e] =
//             #{q : e_q < e} in the same pass. The first two 16 B pieces per
//             thread of row p / k of x are loaded before the scan and stored
//             after it, so the scan hides the row's latency (H <= 4096 is
//             all of the row). Expert ids are clamped to [0, E - 1].
//   moe_combine_kernel      one workgroup per token, 8 columns per thread and
//             trip: out[t] = bf16(sum_j weights[t, j] * float(y[dst[t k + j]]))
//             in ascending j, each product and each sum rounded to fp32 (the
//             kernel body is compiled with contraction off), which for k = 2
//             are the bits of (y.float() * w).sum(1).to(bf16). dst is clamped
//             to [0, P - 1].

#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>

using bf16x8 = __attribute__((ext_vector_type(8))) short;

#define MR_THREADS (4 * WAVE)
#define MR_MAX_E 64
#define MR_MAX_K 8

DEV float dot8(bf16x8 a, bf16x8 b, float acc) {
#pragma unroll
  for (int i = 0; i < 8; ++i) acc += bf2f(a[i]) * bf2f(b[i]);
  return acc;
}

// NCH > 0: the row sits in NCH pieces per lane (H <= 512 * NCH);
// NCH == 0: any H, x is read again for every expert.
template <int NCH>
__global__ void __launch_bounds__(MR_THREADS)
moe_route_kernel(int* __restrict__ experts_out,     // [T, k]
                 float* __restrict__ weights_out,   // [T, k]
                 const short* __restrict__ x,       // [T, H]
                 const short* __restrict__ router,  // [E, H]
                 int H, int E, int k) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const long t = blockIdx.x;
  const int pieces = H >> 3;
  const bf16x8* xrow = (const bf16x8*)(x + t * H);
  __shared__ float s_logit[MR_MAX_E];

  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 xr[NCH > 0 ? NCH : 1];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int i = lane + c * WAVE;
    xr[c] = i < pieces ? xrow[i] : zero8;  // a zero piece adds nothing
  }

  for (int e = wave; e < E; e += 4) {
    const bf16x8* wrow = (const bf16x8*)(router + (long)e * H);
    float acc = 0.f;
    if (NCH > 0) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = lane + c * WAVE;
        acc = dot8(xr[c], wrow[min(i, pieces - 1)], acc);
      }
    } else {
      for (int i = lane; i < pieces; i += WAVE)
        acc = dot8(xrow[i], wrow[i], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) s_logit[e] = acc;
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- one expert per lane: softmax over all E
  const bool live = lane < E;
  const float logit = live ? s_logit[lane] : -INFINITY;
  const float top = wave_max(logit);
  float p = live ? expf(logit - top) : 0.f;
  p = p / wave_sum(p);
  if (!live) p = -1.f;  // below every probability: never picked (k <= E)

  // ---- k rounds of arg-max; lane j keeps the j-th pick
  float my_p = 0.f, sum = 0.f;
  int my_e = 0;
  for (int j = 0; j < k; ++j) {
    float v = p;
    int idx = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(v, off, 64);
      const int oi = __shfl_xor(idx, off, 64);
      if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
      }
    }
    // lane 0's answer for every lane (NaN logits could make lanes differ)
    v = __shfl(v, 0, 64);
    idx = min(__shfl(idx, 0, 64), E - 1);
    if (lane == idx) p = -1.f;
    if (lane == j) {
      my_p = v;
      my_e = idx;
    }
    sum += v;
  }
  if (lane < k) {
    experts_out[t * k + lane] = my_e;
    weights_out[t * k + lane] = my_p / sum;
  }
}

void moe_route(torch::Tensor experts_out, torch::Tensor weights_out,
               torch::Tensor x, torch::Tensor router_w) {
  TORCH_CHECK(x.is_cuda() && router_w.is_cuda() && experts_out.is_cuda() &&
                  weights_out.is_cuda(),
              "moe_route takes device tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.dim() == 2 &&
                  x.is_contiguous(),
              "x must be a contiguous bfloat16 [T, H]");
  const long T = x.size(0), H = x.size(1);
  TORCH_CHECK(H > 0 && H % 8 == 0, "H must be a multiple of 8; got ", H);
  TORCH_CHECK(router_w.scalar_type() == torch::kBFloat16 &&
                  router_w.dim() == 2 && router_w.size(1) == H &&
                  router_w.is_contiguous(),
              "router_w must be a contiguous bfloat16 [E, ", H, "]; got ",
              router_w.sizes());
  const long E = router_w.size(0);
  TORCH_CHECK(E >= 1 && E <= MR_MAX_E, "1 <= E <= 64; got ", E);
  TORCH_CHECK(experts_out.scalar_type() == torch::kInt32 &&
                  experts_out.dim() == 2 && experts_out.size(0) == T &&
                  experts_out.is_contiguous(),
              "experts_out must be a contiguous int32 [", T, ", k]; got ",
              experts_out.sizes());
  const long k = experts_out.size(1);
  TORCH_CHECK(k >= 1 && k <= std::min<long>(E, MR_MAX_K),
              "1 <= k <= min(E, 8); got k=", k, ", E=", E);
  TORCH_CHECK(weights_out.scalar_type() == torch::kFloat32 &&
                  weights_out.dim() == 2 && weights_out.size(0) == T &&
                  weights_out.size(1) == k && weights_out.is_contiguous(),
              "weights_out must be a contiguous float32 [", T, ", ", k,
              "]; got ", weights_out.sizes());
  if (T == 0) return;
  TORCH_CHECK(T < (1L << 31), "problem too large");
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)T), dim3(MR_THREADS), 0,
                       c10::hip::getCurrentHIPStream(),
                       (int*)experts_out.data_ptr(),
                       (float*)weights_out.data_ptr(),
                       (const short*)x.data_ptr(),
                       (const short*)router_w.data_ptr(), (int)H, (int)E,
                       (int)k);
  };
  if (H <= 1024)
    launch(moe_route_kernel<2>);
  else if (H <= 4096)
    launch(moe_route_kernel<8>);
  else if (H <= 8192)
    launch(moe_route_kernel<16>);
  else
    launch(moe_route_kernel<0>);
  HIP_CHECK_LAST();
}

// Sum of a wave-uniform count over the four waves.
DEV int block_total(int wave_count, int* s) {
  if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = wave_count;
  __syncthreads();
  return s[0] + s[1] + s[2] + s[3];
}

__global__ void __launch_bounds__(MR_THREADS)
moe_sort_gather_kernel(short* __restrict__ x_sorted,     // [P, H]
                       int* __restrict__ dst,            // [P]
                       int* __restrict__ counts,         // [E]
                       int* __restrict__ offsets,        // [E]
                       const short* __restrict__ x,      // [T, H]
                       const int* __restrict__ experts,  // [P]
                       int P, int E, int k, int H) {
  const int b = blockIdx.x;  // assignment (b < P) and expert (b < E)
  const int tid = threadIdx.x;
  const int pieces = H >> 3;
  __shared__ int s_cnt[3][4];

  // ---- the row's first pieces, in flight during the scan
  const bf16x8* src = (const bf16x8*)(x + (long)(b < P ? b / k : 0) * H);
  bf16x8 head[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (b < P && tid + j * MR_THREADS < pieces)
      head[j] = src[tid + j * MR_THREADS];

  const int e_p = b < P ? min(max(experts[b], 0), E - 1) : 0;
  int before = 0, same = 0, less = 0;  // wave-uniform
  for (int q0 = 0; q0 < P; q0 += MR_THREADS) {
    const int q = q0 + tid;
    const bool in = q < P;
    const int e_q = in ? min(max(experts[q], 0), E - 1) : 0;
    before += __popcll(
        __ballot(in && (e_q < e_p || (e_q == e_p && q < b))));
    if (b < E) {
      same += __popcll(__ballot(in && e_q == b));
      less += __popcll(__ballot(in && e_q < b));
    }
  }
  if (b < E) {  // workgroup-uniform
    const int n_same = block_total(same, s_cnt[1]);
    const int n_less = block_total(less, s_cnt[2]);
    if (tid == 0) {
      counts[b] = n_same;
      offsets[b] = n_less;
    }
  }
  if (b >= P) return;
  const int row = block_total(before, s_cnt[0]);  // < P: it counts q != b
  if (tid == 0) dst[b] = row;

  bf16x8* out = (bf16x8*)(x_sorted + (long)row * H);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (tid + j * MR_THREADS < pieces)
      out[tid + j * MR_THREADS] = head[j];
  for (int i = tid + 2 * MR_THREADS; i < pieces; i += MR_THREADS)
    out[i] = src[i];
}

void moe_sort_gather(torch::Tensor x_sorted, torch::Tensor dst,
                     torch::Tensor counts, torch::Tensor offsets,
                     torch::Tensor x, torch::Tensor experts) {
  TORCH_CHECK(x.is_cuda() && experts.is_cuda() && x_sorted.is_cuda() &&
                  dst.is_cuda() && counts.is_cuda() && offsets.is_cuda(),
              "moe_sort_gather takes device tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.dim() == 2 &&
                  x.is_contiguous(),
              "x must be a contiguous bfloat16 [T, H]");
  const long T = x.size(0), H = x.size(1);
  TORCH_CHECK(H > 0 && H % 8 == 0, "H must be a multiple of 8; got ", H);
  TORCH_CHECK(experts.scalar_type() == torch::kInt32 && experts.dim() == 2 &&
                  experts.size(0) == T && experts.size(1) >= 1 &&
                  experts.is_contiguous(),
              "experts must be a contiguous int32 [", T, ", k]; got ",
              experts.sizes());
  const long k = experts.size(1), P = T * k;
  TORCH_CHECK(x_sorted.scalar_type() == torch::kBFloat16 &&
                  x_sorted.dim() == 2 && x_sorted.size(0) == P &&
                  x_sorted.size(1) == H && x_sorted.is_contiguous(),
              "x_sorted must be a contiguous bfloat16 [", P, ", ", H,
              "]; got ", x_sorted.sizes());
  TORCH_CHECK(dst.scalar_type() == torch::kInt32 && dst.dim() == 1 &&
                  dst.numel() == P && dst.is_contiguous(),
              "dst must be a contiguous int32 [", P, "]");
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 &&
                  offsets.scalar_type() == torch::kInt32,
              "counts and offsets must be int32");
  const long E = counts.numel();
  TORCH_CHECK(E >= 1 && E <= MR_MAX_E && offsets.numel() == E &&
                  counts.dim() == 1 && offsets.dim() == 1 &&
                  counts.is_contiguous() && offsets.is_contiguous(),
              "counts and offsets must be contiguous [E], 1 <= E <= 64");
  TORCH_CHECK(P < (1L << 31) - MR_THREADS, "problem too large");
  // P == 0 still writes the E zeros of counts and offsets
  hipLaunchKernelGGL(moe_sort_gather_kernel,
                     dim3((unsigned)std::max(P, E)), dim3(MR_THREADS), 0,
                     c10::hip::getCurrentHIPStream(),
                     (short*)x_sorted.data_ptr(), (int*)dst.data_ptr(),
                     (int*)counts.data_ptr(), (int*)offsets.data_ptr(),
                     (const short*)x.data_ptr(),
                     (const int*)experts.data_ptr(), (int)P, (int)E, (int)k,
                     (int)H);
  HIP_CHECK_LAST();
}

__global__ void __launch_bounds__(MR_THREADS)
moe_combine_kernel(short* __restrict__ out,            // [T, H]
                   const short* __restrict__ y,        // [P, H]
                   const int* __restrict__ dst,        // [P]
                   const float* __restrict__ weights,  // [T, k]
                   int P, int k, int H) {
#pragma clang fp contract(off)  // a product is rounded before it is added
  const long t = blockIdx.x;
  for (int c = threadIdx.x * 8; c < H; c += MR_THREADS * 8) {
    float acc[8];
    for (int j = 0; j < k; ++j) {
      const int row = min(max(dst[t * k + j], 0), P - 1);
      const float w = weights[t * k + j];
      const bf16x8 v = *(const bf16x8*)(y + (long)row * H + c);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float prod = w * bf2f(v[i]);
        acc[i] = j == 0 ? prod : acc[i] + prod;
      }
    }
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f2bf(acc[i]);
    *(bf16x8*)(out + t * H + c) = o;
  }
}

void moe_combine(torch::Tensor out, torch::Tensor y, torch::Tensor dst,
                 torch::Tensor weights) {
  TORCH_CHECK(out.is_cuda() && y.is_cuda() && dst.is_cuda() &&
                  weights.is_cuda(),
              "moe_combine takes device tensors");
  TORCH_CHECK(y.scalar_type() == torch::kBFloat16 && y.dim() == 2 &&
                  y.is_contiguous(),
              "y must be a contiguous bfloat16 [P, H]");
  const long P = y.size(0), H = y.size(1);
  TORCH_CHECK(H > 0 && H % 8 == 0, "H must be a multiple of 8; got ", H);
  TORCH_CHECK(weights.scalar_type() == torch::kFloat32 &&
                  weights.dim() == 2 && weights.size(1) >= 1 &&
                  weights.numel() == P && weights.is_contiguous(),
              "weights must be a contiguous float32 [T, k] with T * k = ", P,
              "; got ", weights.sizes());
  const long T = weights.size(0), k = weights.size(1);
  TORCH_CHECK(dst.scalar_type() == torch::kInt32 && dst.dim() == 1 &&
                  dst.numel() == P && dst.is_contiguous(),
              "dst must be a contiguous int32 [", P, "]");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 && out.dim() == 2 &&
                  out.size(0) == T && out.size(1) == H && out.is_contiguous(),
              "out must be a contiguous bfloat16 [", T, ", ", H, "]; got ",
              out.sizes());
  if (T == 0) return;
  TORCH_CHECK(P < (1L << 31), "problem too large");
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)T), dim3(MR_THREADS),
                     0, c10::hip::getCurrentHIPStream(),
                     (short*)out.data_ptr(), (const short*)y.data_ptr(),
                     (const int*)dst.data_ptr(),
                     (const float*)weights.data_ptr(), (int)P, (int)k,
                     (int)H);
  HIP_CHECK_LAST();
}
