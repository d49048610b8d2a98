// 16-bit radiometry (radiometry.py; not in the reference): the kernels that read a uint16 scene cache
// (L, C, H, W) of digital numbers, and the one that writes digital numbers back.  A band's range is range[c] = (lo_c, hi_c), fp32:
//   normalise   x = min(max((float(v) - lo_c) / (hi_c - lo_c), 0), 1)        one correctly rounded fp32 operation per step, the
//   quantise    v = clamp(rint(min(max(x, 0), 1) * (hi_c - lo_c) + lo_c), 0, 65535), NaN -> fill      span formed once, no FMA
// (`__fsub_rn` / `__fdiv_rn` / `__fmul_rn` / `__fadd_rn` are never contracted; rintf rounds half to even).
//
// drs_crop_d4_u16_f32: the batch launch of the 16-bit feed; items and dihedral rule are augment.hip's.  A pixel is no-data when
//   ALL its C stored values equal `nodata`, so a 256-thread block owns one 64 x 64 output tile of one ITEM and walks the item's
//   bands itself (blockIdx.x / .y = the tile, blockIdx.z strides over the items), where augment.hip gives a block one (item,
//   band) plane.  Per tile:
//     1. (only with hr_marked and a nodata value) the tile's source region, `lines` mapping - lane l -> source column l, a wave's
//        rows in turn: a pixel's bands are compared with `nodata` until one differs (one read for almost every pixel) and the
//        verdict goes to an LDS byte per source element;
//     2. per band: the source region is read ROW BY ROW into an LDS tile, in source order, and the output rows are read out of
//        it through the code's index map - for every code, so both global sides stay row-wise under a transposing code and
//        there is one path to keep right - converted, and stored to hr and (with NaN where the verdict says so) hr_marked.
//   Both phases of 2. use augment.hip's `quads` mapping: lane l -> row (l >> 3) & 3 of the wave's four, columns 4 q .. 4 q + 3
//   with q = (l & 7) + 8 (l >> 5); four passes of 16 rows.  A lane issues ONE 8-byte load (16-byte store) where its four elements
//   lie inside the region and its address is aligned for it, else it moves them one by one: decided per lane at run time (x0, W,
//   S and the 2-byte phase of the cache pointer are arbitrary), the same values either way.
//   LDS: one 32-bit word per element, pitch 65 words.  bank = word address mod 32, conflicts counted within a 32-lane half.
//   Row-wise side: a half holds 4 rows x 8 quads, words r * 65 + 4 q + k -> banks r + 4 q + k + const, r < 4, q < 8: 32 distinct.
//   Column-wise side (transposing codes): words (+-(4 q + k)) * 65 +- r -> banks +-(4 q + k) +- r + const: the same 32 values.
//   Pitch 65 = 1 mod 32 makes a step of one LDS row a step of one bank (64 would put a column on one bank: 32-way).
//   No atomics; every output element is written once, by one thread.  An invalid item reads nothing: zeros in both outputs.
//
// drs_hist_u16: exact per-band value counts.  65536 32-bit bins do not fit the LDS (256 KB > 160 KB); 65536 16-BIT bins do (128
//   KB, two to a word, one 1024-thread block per CU).  A work item is (band, up to 65280 consecutive pixels of the band's L
//   planes): no 16-bit bin can overflow inside one item (and no carry can reach the neighbour that shares its word), and the
//   block flushes its non-zero bins to the 64-bit global counts with one atomic each after every item.  The worst case of real
//   scenes - most pixels on a few values, at the limit a constant plane - never reaches global memory pixel by pixel: a wave
//   whose active lanes all hold ONE value adds their number with one LDS atomic from one lane (one ballot); otherwise each lane
//   adds 1 to its bin in LDS.  A plane is walked as head (elements up to the first 16-byte boundary), 16-byte loads of eight
//   values, tail: the 2-byte phase of the pointer and odd plane sizes only move the boundaries.  A value equal to `nodata` makes
//   its thread look at the pixel's other bands (only then), and the pixel is skipped when all agree.  Integer counts: the result
//   does not depend on the order of the atomics.  Measured alternatives: DESIGN.md section 29.
//
// drs_quantize_u16: four consecutive elements per thread, one 16-byte load / 8-byte store where both are aligned for it, else
//   element by element; a group may straddle planes (H W % 4 != 0): the band is tracked per element.
#include "drs_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kPitch = kTile + 1;

constexpr int kHistThreads = 1024;
constexpr int kHistWords = 32768;         // 65536 16-bit bins, two to a word
constexpr long long kHistChunk = 65280;   // pixels per work item: < 65536, a multiple of 256
constexpr int kHistLds = kHistWords * 4;  // 128 KB

__device__ __forceinline__ float unit_from_u16(unsigned v, float lo, float span) {
  return fminf(fmaxf(__fdiv_rn(__fsub_rn((float)v, lo), span), 0.f), 1.f);
}

__device__ __forceinline__ unsigned short u16_from_unit(float x, float lo, float span, unsigned short fill) {
  if (x != x) return fill;
  const float c = fminf(fmaxf(x, 0.f), 1.f);
  const float r = rintf(__fadd_rn(__fmul_rn(c, span), lo));
  return (unsigned short)fminf(fmaxf(r, 0.f), 65535.f);
}

// the `cnt` (1..4) values at p, ascending, into w[0..cnt): one 8-byte access where all four are wanted and p is aligned for it
__device__ __forceinline__ void fetch4(const unsigned short* p, int cnt, unsigned w[4]) {
  if (cnt == 4 && ((uintptr_t)p & 7u) == 0) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    w[0] = v.x & 0xffffu, w[1] = v.x >> 16, w[2] = v.y & 0xffffu, w[3] = v.y >> 16;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) w[k] = p[k];
  }
}

// o[0..cnt) to d: one 16-byte access where all four are written and d is aligned for it
__device__ __forceinline__ void store4(float* d, int cnt, const float o[4]) {
  if (cnt == 4 && ((uintptr_t)d & 15u) == 0) {
    *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) d[k] = o[k];
  }
}

__global__ __launch_bounds__(kThreads) void crop_d4_u16_kernel(const unsigned short* __restrict__ cache,
                                                               const int* __restrict__ items, int n, long long L, int C, int H,
                                                               int W, int S, const float* __restrict__ range, int nodata,
                                                               float* __restrict__ hr, float* __restrict__ hr_marked) {
  __shared__ unsigned tile[kTile * kPitch];
  __shared__ unsigned char nd[kTile * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qrow = (lane >> 3) & 3, qcol = 4 * ((lane & 7) + 8 * (lane >> 5));  // the `quads` mapping
  const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int th = min(kTile, S - ty0), tw = min(kTile, S - tx0);
  const long long plane = (long long)H * W;
  const bool mark = hr_marked != nullptr && nodata >= 0;
  const float nan = __uint_as_float(0x7fc00000u);
  for (int i = blockIdx.z; i < n; i += gridDim.z) {
    const int src = items[4 * i], y0 = items[4 * i + 1], x0 = items[4 * i + 2], code = items[4 * i + 3];
    const bool valid = src >= 0 && src < L && code >= 0 && code < 8 && y0 >= 0 && x0 >= 0 && y0 <= H - S && x0 <= W - S;
    const bool fx = code & 1, fy = code & 2, tr = code & 4;
    float* __restrict__ dst = hr + (((long long)i * C) * S + ty0) * (long long)S + tx0;            // band 0 of the tile
    float* __restrict__ dstm = hr_marked ? hr_marked + (dst - hr) : nullptr;
    const long long out_plane = (long long)S * S;
    if (!valid) {  // reads nothing
      const float z[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C; ++c)
#pragma unroll 1
        for (int pass = 0; pass < kTile / 16; ++pass) {
          const int ly = pass * 16 + wave * 4 + qrow;
          if (ly < th && qcol < tw) {
            const long long o = c * out_plane + (long long)ly * S + qcol;
            store4(dst + o, min(4, tw - qcol), z);
            if (dstm) store4(dstm + o, min(4, tw - qcol), z);
          }
        }
      continue;
    }
    // the tile's source region: sh rows x sw columns from (rs0, cs0) of the window, in source order
    const int sh = tr ? tw : th, sw = tr ? th : tw;
    const int rs0 = tr ? (fx ? S - tx0 - tw : tx0) : (fy ? S - ty0 - th : ty0);
    const int cs0 = tr ? (fy ? S - ty0 - th : ty0) : (fx ? S - tx0 - tw : tx0);
    // band 0 of the region's element (0, 0)
    const unsigned short* __restrict__ reg = cache + ((long long)src * C) * plane + (long long)(y0 + rs0) * W + (x0 + cs0);
    if (mark) {
      for (int sr = wave; sr < sh; sr += kThreads / 64)
        if (lane < sw) {
          const unsigned short* p = reg + (long long)sr * W + lane;
          bool all = true;
          for (int c = 0; c < C; ++c)
            if (p[c * plane] != (unsigned)nodata) {
              all = false;
              break;
            }
          nd[sr * kPitch + lane] = all;
        }
    }
    for (int c = 0; c < C; ++c) {
      const float lo = range[2 * c], span = __fsub_rn(range[2 * c + 1], lo);
      const unsigned short* __restrict__ regc = reg + c * plane;
#pragma unroll 1
      for (int pass = 0; pass < kTile / 16; ++pass) {
        const int sr = pass * 16 + wave * 4 + qrow;
        if (sr < sh && qcol < sw) {
          unsigned w[4];
          fetch4(regc + (long long)sr * W + qcol, min(4, sw - qcol), w);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (qcol + k < sw) tile[sr * kPitch + qcol + k] = w[k];
        }
      }
      __syncthreads();  // (also orders the verdicts of `nd` in front of the first band's read-out)
#pragma unroll 1
      for (int pass = 0; pass < kTile / 16; ++pass) {
        const int ly = pass * 16 + wave * 4 + qrow;
        if (ly < th && qcol < tw) {
          const int cnt = min(4, tw - qcol);
          float o[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < cnt) {
              const int lx = qcol + k;
              const int u = fy ? th - 1 - ly : ly, v = fx ? tw - 1 - lx : lx;  // output (ly, lx) = region (tr ? (v, u) : (u, v))
              const int idx = tr ? v * kPitch + u : u * kPitch + v;
              o[k] = unit_from_u16(tile[idx], lo, span);
              m[k] = mark && nd[idx] ? nan : o[k];
            }
          const long long off = c * out_plane + (long long)ly * S + qcol;
          store4(dst + off, cnt, o);
          if (dstm) store4(dstm + off, cnt, m);
        }
      }
      __syncthreads();  // the tile is filled again for the next band (and `nd` for the block's next item)
    }
  }
}

// one value of band c at pixel `pix` of image l into the block's LDS bins; `take` lanes only (the others idle through it)
__device__ __forceinline__ void hist_add(unsigned* bins, unsigned v) {
  const unsigned long long act = __ballot(1);
  const unsigned first = __builtin_amdgcn_readfirstlane(v);
  if (__ballot(v == first) == act) {  // the wave's active lanes agree: one add of their number
    if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(&bins[first >> 1], (unsigned)__popcll(act) << (16 * (first & 1)));
  } else {
    atomicAdd(&bins[v >> 1], 1u << (16 * (v & 1)));
  }
}

__device__ __forceinline__ bool hist_is_nodata(const unsigned short* __restrict__ image, long long plane, long long pix, int C,
                                               int c, int nodata) {
  for (int k = 0; k < C; ++k)
    if (k != c && image[k * plane + pix] != (unsigned)nodata) return false;
  return true;
}

__global__ __launch_bounds__(kHistThreads) void hist_u16_kernel(const unsigned short* __restrict__ cache, long long L, int C,
                                                                long long plane, int nodata, long long chunks,
                                                                unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned bins[];
  for (int w = threadIdx.x; w < kHistWords; w += kHistThreads) bins[w] = 0u;
  __syncthreads();
  const long long total = L * plane;  // pixels of one band
  for (long long item = blockIdx.x; item < chunks * C; item += gridDim.x) {
    const int c = (int)(item % C);
    const long long p0 = (item / C) * kHistChunk, p1 = min(p0 + kHistChunk, total);
    for (long long l = p0 / plane; l * plane < p1; ++l) {
      const long long a = max(p0 - l * plane, 0ll), b = min(p1 - l * plane, plane);  // pixels [a, b) of image l
      const unsigned short* __restrict__ image = cache + l * C * plane;
      const unsigned short* __restrict__ band = image + c * plane;
      const long long head = min(b - a, (long long)(((16u - ((uintptr_t)(band + a) & 15u)) & 15u) >> 1));
      const long long nvec = (b - a - head) >> 3, tail0 = a + head + 8 * nvec;
      // head and tail: fewer than 8 elements each
      for (int side = 0; side < 2; ++side) {
        const long long pix = (side ? tail0 : a) + threadIdx.x, end = side ? b : a + head;
        if (pix < end) {
          const unsigned v = band[pix];
          if (!(nodata >= 0 && v == (unsigned)nodata && hist_is_nodata(image, plane, pix, C, c, nodata))) hist_add(bins, v);
        }
      }
      for (long long g = threadIdx.x; g < nvec; g += kHistThreads) {
        const long long pix = a + head + 8 * g;
        const uint4 q = *reinterpret_cast<const uint4*>(band + pix);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned v = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
          if (!(nodata >= 0 && v == (unsigned)nodata && hist_is_nodata(image, plane, pix + k, C, c, nodata))) hist_add(bins, v);
        }
      }
    }
    __syncthreads();
    unsigned long long* __restrict__ out = counts + (long long)c * 65536;
    for (int w = threadIdx.x; w < kHistWords; w += kHistThreads) {
      const unsigned two = bins[w];
      if (two) {
        bins[w] = 0u;
        if (two & 0xffffu) atomicAdd(out + 2 * w, (unsigned long long)(two & 0xffffu));
        if (two >> 16) atomicAdd(out + 2 * w + 1, (unsigned long long)(two >> 16));
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void quantize_u16_kernel(const float* __restrict__ x, long long total, int C, long long HW,
                                                           const float* __restrict__ range, unsigned short fill,
                                                           unsigned short* __restrict__ out) {
  const long long groups = (total + 3) >> 2;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long e0 = 4 * g;
    const int cnt = (int)min(4ll, total - e0);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (cnt == 4 && ((uintptr_t)(x + e0) & 15u) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(x + e0);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) v[k] = x[e0 + k];
    }
    long long p = e0 / HW;          // the (image, band) plane of element e0
    long long r = e0 - p * HW;      // and its place in it
    unsigned short o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) {
        while (r >= HW) r -= HW, ++p;
        const int c = (int)(p % C);
        const float lo = range[2 * c];
        o[k] = u16_from_unit(v[k], lo, __fsub_rn(range[2 * c + 1], lo), fill);
        ++r;
      }
    if (cnt == 4 && ((uintptr_t)(out + e0) & 7u) == 0) {
      *reinterpret_cast<uint2*>(out + e0) = make_uint2((unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) out[e0 + k] = o[k];
    }
  }
}

}  // namespace

extern "C" int drs_crop_d4_u16_f32(const uint16_t* cache_u16, const int32_t* items, int n, int64_t L, int C, int H, int W, int S,
                                   const float* range, int nodata, float* hr, float* hr_marked, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(cache_u16 && items && range && hr, DRS_ERR_ARG, "crop_d4_u16_f32: null pointer");
  DRS_REQUIRE(((uintptr_t)cache_u16 & 1u) == 0, DRS_ERR_ARG, "crop_d4_u16_f32: the cache is not 2-byte aligned");
  DRS_REQUIRE(hr_marked != hr, DRS_ERR_ARG, "crop_d4_u16_f32: hr_marked is hr");
  DRS_REQUIRE(nodata >= -1 && nodata <= 65535, DRS_ERR_ARG, "crop_d4_u16_f32: nodata=%d must be -1 (none) or 0 .. 65535", nodata);
  DRS_REQUIRE(n >= 1 && L >= 1 && C >= 1 && C <= kMaxBands && H >= 1 && W >= 1 && S >= 1 && S <= H && S <= W, DRS_ERR_SHAPE,
              "crop_d4_u16_f32: n=%d L=%lld bands=%d H=%d W=%d S=%d (need n, L >= 1, 1 <= bands <= %d and 1 <= S <= H, W)", n,
              (long long)L, C, H, W, S, kMaxBands);
  const unsigned t = (unsigned)((S + kTile - 1) / kTile);
  DRS_REQUIRE(t <= 65535, DRS_ERR_SHAPE, "crop_d4_u16_f32: S=%d is more than 65535 tiles on a side", S);
  DRS_LAUNCH(crop_d4_u16_kernel, dim3(t, t, (unsigned)(n > 65535 ? 65535 : n)), dim3(kThreads), 0, s,
             (const unsigned short*)cache_u16, (const int*)items, n, (long long)L, C, H, W, S, range, nodata, hr, hr_marked);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_hist_u16(const uint16_t* cache_u16, int64_t L, int C, int H, int W, int nodata, uint64_t* counts,
                            drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(cache_u16 && counts, DRS_ERR_ARG, "hist_u16: null pointer");
  DRS_REQUIRE(((uintptr_t)cache_u16 & 1u) == 0 && ((uintptr_t)counts & 7u) == 0, DRS_ERR_ARG,
              "hist_u16: the cache is not 2-byte aligned or the counts are not 8-byte aligned");
  DRS_REQUIRE(nodata >= -1 && nodata <= 65535, DRS_ERR_ARG, "hist_u16: nodata=%d must be -1 (none) or 0 .. 65535", nodata);
  DRS_REQUIRE(L >= 1 && C >= 1 && C <= kMaxBands && H >= 1 && W >= 1, DRS_ERR_SHAPE,
              "hist_u16: L=%lld bands=%d H=%d W=%d (need L, H, W >= 1 and 1 <= bands <= %d)", (long long)L, C, H, W, kMaxBands);
  const long long plane = (long long)H * W;
  DRS_REQUIRE(L <= (1ll << 40) / plane, DRS_ERR_SHAPE, "hist_u16: L=%lld images of %d x %d are more than 2^40 pixels per band",
              (long long)L, H, W);
  int num_cu = 0;
  const int st = drs_kernel_prepare(reinterpret_cast<const void*>(hist_u16_kernel), kHistLds, &num_cu);
  if (st != DRS_OK) return st;
  DRS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)C * 65536 * sizeof(uint64_t), s));
  const long long chunks = (L * plane + kHistChunk - 1) / kHistChunk;
  const long long blocks = std::min<long long>(chunks * C, std::max(num_cu, 1));
  DRS_LAUNCH(hist_u16_kernel, dim3((unsigned)blocks), dim3(kHistThreads), kHistLds, s, (const unsigned short*)cache_u16,
             (long long)L, C, plane, nodata, chunks, (unsigned long long*)counts);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_quantize_u16(const float* x, int n, int C, int64_t HW, const float* range, int fill, uint16_t* out,
                                drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(x && range && out, DRS_ERR_ARG, "quantize_u16: null pointer");
  DRS_REQUIRE(((uintptr_t)out & 1u) == 0, DRS_ERR_ARG, "quantize_u16: out is not 2-byte aligned");
  DRS_REQUIRE(fill >= 0 && fill <= 65535, DRS_ERR_ARG, "quantize_u16: fill=%d must lie in 0 .. 65535", fill);
  DRS_REQUIRE(n >= 1 && C >= 1 && C <= kMaxBands && HW >= 1, DRS_ERR_SHAPE,
              "quantize_u16: n=%d bands=%d HW=%lld (need n, HW >= 1 and 1 <= bands <= %d)", n, C, (long long)HW, kMaxBands);
  DRS_REQUIRE(HW <= (1ll << 40) / ((long long)n * C), DRS_ERR_SHAPE, "quantize_u16: n=%d x %d planes of %lld are more than 2^40 elements",
              n, C, (long long)HW);
  const long long total = (long long)n * C * HW;
  DRS_LAUNCH(quantize_u16_kernel, dim3(ew_blocks((total + 3) / 4)), dim3(256), 0, s, x, total, C, (long long)HW, range,
             (unsigned short)fill, (unsigned short*)out);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
