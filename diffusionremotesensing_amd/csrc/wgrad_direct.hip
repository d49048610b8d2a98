// Weight gradients of the tap convolutions (reference loop body train_diffusion_superres.py:388-393: loss.backward()):
// drs_launch_wgrad hands a layer to the bf16 / fp32 MFMA kernels (wgrad_mfma_bf16.hip, wgrad_mfma.hip) where they apply
// and to the direct fp32 kernel below (LDS tiles, float atomics across position chunks) where they do not.
#include "drs_common.h"

// ---------------------------------------------------------------------------------------------------------------
// Weight gradient of a tap convolution ("correlation" of two channels-last tensors):
//   dW[tap][a][b] = sum_{n, ty, tx} A[n][ty*sa + ay(tap)][tx*sa + ax(tap)][a] * B[n][ty*sb + by(tap)][tx*sb + bx(tap)][b]
// with zero outside either tensor.  Regular conv: A = layer input (sa = stride, offsets = tap offsets), B = dY (sb = 1);
// transposed conv: A = layer input at (ty, tx), B = dY at (2*ty - 1 + ky, 2*tx - 1 + kx).
// Optional: a_add[n][a] added to in-image A pixels (UpConvBlock adds the time embedding before its conv),
// a_gate[n][y/2][x/2] multiplied into A (the attention gate multiplies x before the `result` conv).
// Output index = out_transposed ? (a*Cb + b)*T + tap : (b*Ca + a)*T + tap  (torch ConvTranspose2d / Conv2d layout).
// grid = (position chunks, taps, (Ca/64)*(Cb/64) tiles); block 256 threads; thread = 4x4 block of (a, b).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wgrad_kernel(WgradDesc d, int chunk) {
  constexpr int TP = 16;  // positions per LDS tile
  __shared__ float sA[TP][64 + 1];
  __shared__ float sB[TP][64 + 1];
  const int tap = blockIdx.y;
  const int tiles_b = (d.Cb + 63) / 64;
  const int a0 = (blockIdx.z / tiles_b) * 64, b0 = (blockIdx.z % tiles_b) * 64;
  const int ta = (threadIdx.x >> 4) * 4, tb = (threadIdx.x & 15) * 4;  // this thread's 4x4 block inside the 64x64 tile
  const long long P = (long long)d.N * d.TH * d.TW;
  const long long p_begin = (long long)blockIdx.x * chunk, p_end = min(P, p_begin + chunk);
  float acc[4][4] = {};
  for (long long p0 = p_begin; p0 < p_end; p0 += TP) {
    // stage TP positions x 64 channels of A and of B (zero outside the image / channel range / chunk)
    for (int i = threadIdx.x; i < TP * 64; i += 256) {
      const int pp = i >> 6, c = i & 63;
      const long long p = p0 + pp;
      float va = 0.f, vb = 0.f;
      if (p < p_end) {
        const int tx = (int)(p % d.TW), ty = (int)((p / d.TW) % d.TH), n = (int)(p / ((long long)d.TW * d.TH));
        const int ya = ty * d.sa + d.ay[tap], xa = tx * d.sa + d.ax[tap];
        const int yb = ty * d.sb + d.by[tap], xb = tx * d.sb + d.bx[tap];
        if (a0 + c < d.Ca && ya >= 0 && ya < d.AH && xa >= 0 && xa < d.AW) {
          va = d.A[(((long long)n * d.AH + ya) * d.AW + xa) * d.a_cs + d.a_co + a0 + c];
          if (d.a_add) va += d.a_add[(long long)n * d.a_add_cs + a0 + c];
          if (d.a_gate) va *= d.a_gate[((long long)n * (d.AH >> 1) + (ya >> 1)) * (d.AW >> 1) + (xa >> 1)];
        }
        if (b0 + c < d.Cb && yb >= 0 && yb < d.BH && xb >= 0 && xb < d.BW)
          vb = d.B[(((long long)n * d.BH + yb) * d.BW + xb) * d.b_cs + d.b_co + b0 + c];
      }
      sA[pp][c] = va;
      sB[pp][c] = vb;
    }
    __syncthreads();
#pragma unroll
    for (int pp = 0; pp < TP; ++pp) {
      float av[4], bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { av[j] = sA[pp][ta + j]; bv[j] = sB[pp][tb + j]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int a = a0 + ta + i, b = b0 + tb + j;
      if (a < d.Ca && b < d.Cb) {
        const long long idx = d.out_transposed ? ((long long)a * d.Cb + b) * d.T_total + d.wtap[tap]
                                               : ((long long)b * d.Ca + a) * d.T_total + d.wtap[tap];
        atomicAdd(&d.dW[idx], acc[i][j]);
      }
    }
}

int drs_launch_wgrad(const WgradDesc& d, hipStream_t s) {
  const long long P = (long long)d.N * d.TH * d.TW;
  if (P == 0) return DRS_OK;
  if (d.partial && drs_wgrad_mfma_bf16_supported(d)) return drs_launch_wgrad_mfma_bf16(d, d.partial, d.partial_bytes, s);
  if (d.partial && drs_wgrad_mfma_supported(d)) return drs_launch_wgrad_mfma(d, d.partial, d.partial_bytes, s);
  if (d.dbias) {  // the direct kernel has no fused bias gradient
    int rc = drs_launch_colsum(d.B, d.b_cs, d.b_co, d.Cb, (long long)d.N * d.BH * d.BW, (long long)d.BH * d.BW, 0, 0, d.dbias, s);
    if (rc) return rc;
  }
  const int tiles = ((d.Ca + 63) / 64) * ((d.Cb + 63) / 64);
  // enough position chunks to fill the chip (~2048 blocks in all), at least 256 positions each
  long long chunks = 2048 / ((long long)d.ntaps * tiles);
  if (chunks < 1) chunks = 1;
  long long chunk = (P + chunks - 1) / chunks;
  if (chunk < 256) chunk = 256;
  chunk = (chunk + 15) / 16 * 16;
  chunks = (P + chunk - 1) / chunk;
  DRS_LAUNCH(wgrad_kernel, dim3((unsigned)chunks, d.ntaps, tiles), dim3(256), 0, s, d, (int)chunk);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
