// Backward of the time-embedding MLPs (reference UNet_model_superres.py:143-151,:161), all of them in one launch.
#include "drs_common.h"

// ---------------------------------------------------------------------------------------------------------------
// Time-embedding MLP backward (reference :143-151,:161): out = relu(W2 silu(W1 e + b1) + b2), e = posenc(t) (constant).
// dim/8 blocks per MLP, each owning 8 rows of every gradient; loops over the batch.  dtemb = gradient w.r.t. out
// (already summed over pixels by the caller).  Each of dW1 / db1 / dW2 / db2 of an MLP and dlabel may be null (the caller
// does not want it): every store tests its own pointer, block-uniformly.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void time_mlp_bwd_kernel(const long long* __restrict__ t,
                                                           const float* __restrict__ inv_freq, DrsMlpBwdTable tab,
                                                           int stride, int B, const float* __restrict__ label_emb,
                                                           const long long* __restrict__ labels, int label_batch,
                                                           int num_classes, float* __restrict__ dlabel) {
  // blockIdx.y = which of the network's time MLPs (all of them in ONE launch: they were seven 73 us launches, each a
  // handful of latency-bound blocks, at the end of the backward's main stream)
  const DrsMlpBwd& e_ = tab.m[blockIdx.y];
  const int dim = e_.dim;
  if ((int)blockIdx.x * 8 >= dim) return;
  const float* __restrict__ W1 = e_.W1;
  const float* __restrict__ b1 = e_.b1;
  const float* __restrict__ W2 = e_.W2;
  const float* __restrict__ temb = e_.temb;
  const float* __restrict__ dtemb = e_.dtemb;
  float* __restrict__ dW1 = e_.dW1;
  float* __restrict__ db1 = e_.db1;
  float* __restrict__ dW2 = e_.dW2;
  float* __restrict__ db2 = e_.db2;
  // Block `blockIdx.x` owns rows [r0, r0 + RB) of dW2 / db2 (index c) and of dW1 / db1 (index k): it re-derives the
  // cheap per-sample vectors (e, pre1, h1, d2: dim x 100 MACs) and keeps its rows' sums over the batch in registers.
  constexpr int RB = 8;
  __shared__ float e[100], pre1[256], h1[256], d2[256], dpre1[RB];
  const int r0 = blockIdx.x * RB;
  const int tid = threadIdx.x;
  float acc2[RB], acc1[RB], accb2 = 0.f, accb1 = 0.f;
#pragma unroll
  for (int r = 0; r < RB; ++r) acc2[r] = acc1[r] = 0.f;
  for (int b = 0; b < B; ++b) {
    const float tf = (float)t[b];
    long long lab = labels ? labels[label_batch == 1 ? 0 : b] : 0;
    if (lab >= num_classes) lab = -1;  // out-of-range class id (the forward poisoned that row with NaN): never index with it
    if (tid < 50) {
      const float arg = tf * inv_freq[tid];
      e[tid] = sinf(arg);
      e[50 + tid] = cosf(arg);
    }
    __syncthreads();
    if (labels) {  // e = posenc(t) + label_emb[y] (generation variant)
      if (tid < 100 && lab >= 0) e[tid] += label_emb[lab * 100 + tid];
      __syncthreads();
    }
    if (tid < dim) {
      float a = b1[tid];
      for (int k = 0; k < 100; ++k) a = fmaf(W1[(size_t)tid * 100 + k], e[k], a);
      pre1[tid] = a;
      h1[tid] = a / (1.f + expf(-a));
      d2[tid] = temb[(size_t)b * stride + tid] > 0.f ? dtemb[(size_t)b * stride + tid] : 0.f;  // ReLU mask
    }
    __syncthreads();
    {  // dpre1[k] = silu'(pre1[k]) * sum_c W2[c][k] d2[c] for this block's RB rows k: 32 lanes per row
      const int rr = tid >> 5, l = tid & 31, k = r0 + rr;
      float dh = 0.f;
      if (k < dim)
        for (int c = l; c < dim; c += 32) dh = fmaf(W2[(size_t)c * dim + k], d2[c], dh);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) dh += __shfl_xor(dh, o, 32);
      if (l == 0) {
        float v = 0.f;
        if (k < dim) {
          const float sg = 1.f / (1.f + expf(-pre1[k]));
          v = dh * (sg * (1.f + pre1[k] * (1.f - sg)));  // d silu
        }
        dpre1[rr] = v;
      }
    }
    __syncthreads();
    if (tid < dim) {
#pragma unroll
      for (int r = 0; r < RB; ++r) acc2[r] = fmaf(r0 + r < dim ? d2[r0 + r] : 0.f, h1[tid], acc2[r]);
    }
    if (tid < 100) {
#pragma unroll
      for (int r = 0; r < RB; ++r) acc1[r] = fmaf(dpre1[r], e[tid], acc1[r]);
      if (dlabel && lab >= 0) {  // d e = W1^T dpre1: this block's RB rows of the sum, onto the embedding row of the sample's class
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < RB; ++r)
          if (r0 + r < dim) a = fmaf(W1[(size_t)(r0 + r) * 100 + tid], dpre1[r], a);
        atomicAdd(&dlabel[lab * 100 + tid], a);
      }
    }
    if (tid >= 128 && tid < 128 + RB) {
      const int r = tid - 128;
      if (r0 + r < dim) { accb2 += d2[r0 + r]; accb1 += dpre1[r]; }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r0 + r >= dim) break;
    if (dW2 && tid < dim) dW2[(size_t)(r0 + r) * dim + tid] += acc2[r];
    if (dW1 && tid < 100) dW1[(size_t)(r0 + r) * 100 + tid] += acc1[r];
  }
  if (tid >= 128 && tid < 128 + RB && r0 + tid - 128 < dim) {
    if (db2) db2[r0 + tid - 128] += accb2;
    if (db1) db1[r0 + tid - 128] += accb1;
  }
}
int drs_launch_time_mlp_bwd(const long long* t, const float* inv_freq, const DrsMlpBwdTable& tab, int stride, int B,
                            const float* label_emb, const long long* labels, int label_batch, int num_classes, float* dlabel,
                            hipStream_t s) {
  if (tab.n == 0) return DRS_OK;
  int max_dim = 0;
  for (int i = 0; i < tab.n; ++i) {
    DRS_REQUIRE(tab.m[i].dim <= 256, DRS_ERR_SHAPE, "time_mlp_bwd: dim=%d", tab.m[i].dim);
    max_dim = tab.m[i].dim > max_dim ? tab.m[i].dim : max_dim;
  }
  // (the label-embedding gradient is accumulated with atomics by every MLP's blocks, as before)
  DRS_LAUNCH(time_mlp_bwd_kernel, dim3((max_dim + 7) / 8, tab.n), dim3(256), 0, s, t, inv_freq, tab, stride, B, label_emb, labels,
             label_batch, num_classes, dlabel);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
