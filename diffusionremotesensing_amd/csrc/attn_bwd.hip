// Backward of the attention gate and of its psi convolution (reference AttentionBlock, UNet_model_superres.py:78,:104-107).
#include "drs_common.h"

// ---------------------------------------------------------------------------------------------------------------
// Attention gate backward (reference AttentionBlock :104-107).  Forward: Zr = up2(psi) * (Wr x) + br.
// With E = Wr^T dZr (a 1x1 dgrad, computed by the caller):
//   dpsi_pre[n][y][x] = psi (1 - psi) * sum_{2x2} sum_c x[n][2y+a][2x+b][c] * E[...][c]
//   dx[n][Y][X][c] += psi[n][Y/2][X/2] * E[n][Y][X][c]
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ x, const float* __restrict__ E,
                                                       const float* __restrict__ psi, float* __restrict__ dx,
                                                       float* __restrict__ dpsi_pre, int N, int LH, int LW, int C) {
  // one wave per low-resolution position: lanes stride the 4*C products
  const int lane = threadIdx.x & 63;
  const long long pos = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long total = (long long)N * LH * LW;
  if (pos >= total) return;
  const int lx = (int)(pos % LW), ly = (int)((pos / LW) % LH), n = (int)(pos / ((long long)LW * LH));
  const float ps = psi[pos];
  float s = 0.f;
  for (int i = lane; i < 4 * C; i += 64) {
    const int sub = i / C, c = i - sub * C;
    const long long hp = (((long long)n * 2 * LH + 2 * ly + (sub >> 1)) * 2 * LW + 2 * lx + (sub & 1)) * C + c;
    const float e = E[hp];
    s += x[hp] * e;
    dx[hp] += ps * e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) dpsi_pre[pos] = s * ps * (1.f - ps);
}
int drs_launch_gate_bwd(const float* x, const float* E, const float* psi, float* dx, float* dpsi_pre, int N, int LH,
                        int LW, int C, hipStream_t s) {
  const long long total = (long long)N * LH * LW;
  DRS_LAUNCH(gate_bwd_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, x, E, psi, dx, dpsi_pre, N, LH, LW,
                     C);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// psi conv backward (1x1 conv to one channel, reference :78,:104):  psi_pre = sum_c wpsi[c] P[p][c] + b.
//   dP[p][c] = wpsi[c] * dpsi_pre[p] * (P[p][c] > 0)   (P is a ReLU output: its mask is applied here)
//   dw[c] += sum_p P[p][c] * dpsi_pre[p],  db += sum_p dpsi_pre[p]
// thread = (pixel row in block, group of 4 channels); the block's sums go to ITS row of `partials` ([C] dw | db), the finish
// kernel adds the rows into dw / db (no atomics onto C + 1 shared addresses: see bn_stats_kernel)
__global__ __launch_bounds__(256) void psi_bwd_kernel(const float* __restrict__ Pm, const float* __restrict__ wpsi,
                                                      const float* __restrict__ dpsi_pre, float* __restrict__ dP,
                                                      float* __restrict__ partials, int C, long long npix, int rows_per_block) {
  __shared__ float red[256][5];
  const int c4n = C >> 2, rows = 256 / c4n;
  const int q = threadIdx.x % c4n, row = threadIdx.x / c4n;
  const long long p_begin = (long long)blockIdx.x * rows_per_block, p_end = min(npix, p_begin + rows_per_block);
  float sw[4] = {0.f, 0.f, 0.f, 0.f}, sb = 0.f;
  if (row < rows) {
    const float4 w = *reinterpret_cast<const float4*>(wpsi + q * 4);
    for (long long p = p_begin + row; p < p_end; p += rows) {
      const float dp = dpsi_pre[p];
      const float4 pv = *reinterpret_cast<const float4*>(Pm + p * C + q * 4);
      *reinterpret_cast<float4*>(dP + p * C + q * 4) =
          make_float4(pv.x > 0.f ? w.x * dp : 0.f, pv.y > 0.f ? w.y * dp : 0.f, pv.z > 0.f ? w.z * dp : 0.f, pv.w > 0.f ? w.w * dp : 0.f);
      sw[0] += pv.x * dp; sw[1] += pv.y * dp; sw[2] += pv.z * dp; sw[3] += pv.w * dp;
      if (q == 0) sb += dp;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[threadIdx.x][j] = sw[j];
  red[threadIdx.x][4] = sb;
  __syncthreads();
  if (threadIdx.x < c4n) {
    float* prow = partials + (size_t)blockIdx.x * (C + 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = 0.f;
      for (int r = 0; r < rows; ++r) v += red[r * c4n + threadIdx.x][j];
      prow[threadIdx.x * 4 + j] = v;
    }
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int r = 0; r < rows; ++r) t += red[r * c4n][4];
      prow[C] = t;
    }
  }
}
int drs_launch_psi_bwd(const float* Pm, const float* wpsi, const float* dpsi_pre, float* dP, float* dw, float* db, int C,
                       long long npix, float* partials, hipStream_t s) {
  // partials: at most 2048 rows of C + 1 floats of scratch (stream-ordered use)
  DRS_REQUIRE(C % 4 == 0 && C <= 256 && 256 % (C >> 2) == 0, DRS_ERR_SHAPE, "psi_bwd: C=%d", C);
  if (npix == 0) return DRS_OK;
  long long rpb = 256;
  while ((npix + rpb - 1) / rpb > 2048) rpb *= 2;
  const unsigned blocks = (unsigned)((npix + rpb - 1) / rpb);
  DRS_LAUNCH(psi_bwd_kernel, dim3(blocks), dim3(256), 0, s, Pm, wpsi, dpsi_pre, dP, partials, C, npix, (int)rpb);
  return drs_launch_rows_finish(partials, (int)blocks, C + 1, C, dw, db, s);  // column C = the bias gradient
}
