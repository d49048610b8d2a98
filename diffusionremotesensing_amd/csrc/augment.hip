// Random crops and dihedral augmentation of the device feeds (augment.py): one launch writes a whole batch.  Item i is
// items[i] = (src, y0, x0, code): the S x S window of cache image `src` with top-left corner (y0, x0), under dihedral code 0..7
//   if code & 4: w = w.swapaxes(-1, -2)     # transpose first
//   if code & 1: w = w[..., ::-1]           # then reverse the columns
//   if code & 2: w = w[..., ::-1, :]        # then reverse the rows
// i.e. out[i, c, y, x] = cache[src, c, y0 + y', x0 + x'] with (u, v) = (code & 2 ? S-1-y : y, code & 1 ? S-1-x : x) and
// (y', x') = code & 4 ? (v, u) : (u, v); all bands of an item (and both tensors of a pair) share window and code.
// Three output forms: the bytes themselves, float(b) / 255 (+ the item's label), (v + 1) * 0.5 for the two tensors of a pair.
// An item whose src, window or code is out of range reads nothing: zeros (label -1), the convention of feed.hip.
//
// Layout.  A 256-thread block owns one 64 x 64 output tile of one (item, band) plane: blockIdx.x / .y = the tile, blockIdx.z
// strides over the n * bands planes.  The tile is walked in four passes of 16 rows, a wave taking four rows per pass, in one
// of two lane mappings:
//   quads   lane l -> row (l >> 3) & 3, columns 4 q .. 4 q + 3 with q = (l & 7) + 8 (l >> 5): one 4-element vector access per
//           lane (4 bytes / 16 bytes), runs of 8 lanes on consecutive addresses.  A vector access is issued only by a lane
//           whose four elements lie inside the tile (hence inside the window's row) and whose address is aligned for it;
//           every other lane of the mapping moves its elements one by one.
//   lines   lane l -> column l, the wave's four rows in turn: element accesses, 64 lanes on consecutive addresses.
// `quads` is chosen per tile and side where the side's tile origin is aligned for the vector and its row pitch keeps that
// alignment from row to row (feed.hip's rule: decided at run time, x0 / S / the pitches are arbitrary); else `lines`.
//   code & 4 == 0: an output row is a segment of one source row, forwards or backwards: each lane loads its four sources
//     (the reversal lives in the addresses and in the order of the four registers) and stores them.  No LDS.
//   code & 4 != 0: the tile's source region (tw source rows x th source columns) is read ROW BY ROW into an LDS tile, in
//     source order, and the output rows are read out of it COLUMN-wise: both global sides stay row-wise.  The row and column
//     reversals are index arithmetic on the LDS side.
// LDS: one 32-bit word per element (bytes widened), pitch 65 words.  Every access is a ds_write_b32 / ds_read_b32: bank =
// word address mod 32, conflicts counted within each 32-lane half.  Row-wise side: `quads` puts a half on 4 rows x 8 quads,
// words r * 65 + 4 q + k -> banks r + 4 q + k + const, r < 4, q < 8: 32 distinct; `lines` on 32 consecutive words.  Column-wise
// side: `quads` reads words (+-(4 q + k)) * 65 +- r -> banks +-(4 q + k) +- r + const, again the 32 values r + 4 q; `lines`
// reads words +-l * 65 -> banks +-l + const.  Pitch 65 = 1 mod 32 is what makes a step of one LDS row a step of one bank (64
// would put a column on one bank: 32-way).  No atomics; every output element is written once, by one thread.
// The pass loops stay rolled (`#pragma unroll 1`): unrolled, the compiler keeps all four passes' addresses and data live (205
// VGPRs, 2 waves per SIMD) and the kernel takes 1.5 - 2x as long as at the 71 - 78 VGPRs (6 - 7 waves) of the rolled form, measured.
#include "drs_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kPitch = kTile + 1;

__device__ __forceinline__ float unit_from_pm1(float v) {
#pragma clang fp contract(off)
  return (v + 1.0f) * 0.5f;
}

__device__ __forceinline__ float unit_from_u8(unsigned b) { return __fdiv_rn((float)b, 255.f); }

struct CopyU8 {
  typedef unsigned char In;
  typedef unsigned char Out;
  static __device__ __forceinline__ unsigned char apply(unsigned w) { return (unsigned char)w; }
};
struct UnitU8 {
  typedef unsigned char In;
  typedef float Out;
  static __device__ __forceinline__ float apply(unsigned w) { return unit_from_u8(w); }
};
struct UnitPm1 {
  typedef float In;
  typedef float Out;
  static __device__ __forceinline__ float apply(unsigned w) { return unit_from_pm1(__uint_as_float(w)); }
};

// an element as the 32-bit word the kernel carries it in (and keeps it in LDS)
__device__ __forceinline__ unsigned word_of(unsigned char b) { return b; }
__device__ __forceinline__ unsigned word_of(float v) { return __float_as_uint(v); }

template <typename T>
__device__ __forceinline__ bool aligned4(const T* p) { return ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0; }

// four consecutive elements in one access; p is aligned4
__device__ __forceinline__ void load4(const unsigned char* p, unsigned w[4]) {
  const unsigned v = *reinterpret_cast<const unsigned*>(p);
  w[0] = v & 0xffu, w[1] = (v >> 8) & 0xffu, w[2] = (v >> 16) & 0xffu, w[3] = v >> 24;
}
__device__ __forceinline__ void load4(const float* p, unsigned w[4]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  w[0] = __float_as_uint(v.x), w[1] = __float_as_uint(v.y), w[2] = __float_as_uint(v.z), w[3] = __float_as_uint(v.w);
}
__device__ __forceinline__ void store4(unsigned char* p, unsigned char a, unsigned char b, unsigned char c, unsigned char d) {
  *reinterpret_cast<unsigned*>(p) = (unsigned)a | ((unsigned)b << 8) | ((unsigned)c << 16) | ((unsigned)d << 24);
}
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

// the `cnt` (1..4) elements at p, ascending, into w[0..cnt): one access where all four are wanted and p is aligned for it
template <typename T>
__device__ __forceinline__ void fetch4(const T* p, int cnt, unsigned w[4]) {
  if (cnt == 4 && aligned4(p)) {
    load4(p, w);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) w[k] = word_of(p[k]);
  }
}

// w[0..cnt) converted (zeros when !valid) to d[0..cnt); one access where all four are written and d is aligned for it
template <typename Cv>
__device__ __forceinline__ void emit4(typename Cv::Out* d, int cnt, const unsigned w[4], bool valid) {
  typedef typename Cv::Out Out;
  Out o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = valid ? Cv::apply(w[k]) : Out(0);
  if (cnt == 4 && aligned4(d)) {
    store4(d, o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) d[k] = o[k];
  }
}

template <typename Cv>
struct Side {
  const typename Cv::In* cache;  // (L, bands, H, W)
  typename Cv::Out* out;         // (n, bands, S, S)
  int bands;
};

template <typename Cv>
__global__ __launch_bounds__(kThreads) void crop_d4_kernel(Side<Cv> a, Side<Cv> b, const int* __restrict__ items, int n,
                                                           long long L, int H, int W, int S,
                                                           const long long* __restrict__ labels,
                                                           long long* __restrict__ labels_out) {
  typedef typename Cv::In In;
  typedef typename Cv::Out Out;
  __shared__ unsigned tile[kTile * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qrow = (lane >> 3) & 3, qcol = 4 * ((lane & 7) + 8 * (lane >> 5));  // the `quads` mapping
  const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int th = min(kTile, S - ty0), tw = min(kTile, S - tx0);
  const int bands = a.bands + b.bands;
  const long long planes = (long long)n * bands;
  for (long long p = blockIdx.z; p < planes; p += gridDim.z) {
    const int i = (int)(p / bands), band = (int)(p - (long long)i * bands);
    const bool second = band >= a.bands;
    const int c = second ? band - a.bands : band, C = second ? b.bands : a.bands;
    const int src = items[4 * i], y0 = items[4 * i + 1], x0 = items[4 * i + 2], code = items[4 * i + 3];
    const bool valid = src >= 0 && src < L && code >= 0 && code < 8 && y0 >= 0 && x0 >= 0 && y0 <= H - S && x0 <= W - S;
    if (labels_out && band == 0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
      labels_out[i] = valid ? labels[src] : -1;
    // the window's element (0, 0); an invalid item's pointer is never dereferenced
    const In* __restrict__ win = (second ? b.cache : a.cache) +
                                 (valid ? (((long long)src * C + c) * H + y0) * (long long)W + x0 : 0);
    Out* __restrict__ dst = (second ? b.out : a.out) + (((long long)i * C + c) * S + ty0) * (long long)S + tx0;
    const bool fx = code & 1, fy = code & 2, tr = valid && (code & 4);
    const bool out_quads = aligned4(dst) && (S * sizeof(Out)) % (4 * sizeof(Out)) == 0;

    if (tr) {
      // the source region of this tile: rows rs0 .. rs0 + tw (one per output column), columns cs0 .. cs0 + th, in source order
      const int rs0 = fx ? S - tx0 - tw : tx0, cs0 = fy ? S - ty0 - th : ty0;
      const In* __restrict__ reg = win + (long long)rs0 * W + cs0;
      if (aligned4(reg) && (W * sizeof(In)) % (4 * sizeof(In)) == 0) {
#pragma unroll 1
        for (int pass = 0; pass < kTile / 16; ++pass) {
          const int sr = pass * 16 + wave * 4 + qrow;
          if (sr < tw && qcol < th) {
            unsigned w[4];
            fetch4(reg + (long long)sr * W + qcol, min(4, th - qcol), w);
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (qcol + k < th) tile[sr * kPitch + qcol + k] = w[k];
          }
        }
      } else {
#pragma unroll 1
        for (int pass = 0; pass < kTile / 16; ++pass)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int sr = pass * 16 + wave * 4 + k;
            if (sr < tw && lane < th) tile[sr * kPitch + lane] = word_of(reg[(long long)sr * W + lane]);
          }
      }
      __syncthreads();
      // output (ly, lx) of the tile = region element (row fx ? tw-1-lx : lx, column fy ? th-1-ly : ly)
      if (out_quads) {
#pragma unroll 1
        for (int pass = 0; pass < kTile / 16; ++pass) {
          const int ly = pass * 16 + wave * 4 + qrow;
          if (ly < th && qcol < tw) {
            const int sc = fy ? th - 1 - ly : ly;
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (qcol + k < tw) w[k] = tile[(fx ? tw - 1 - qcol - k : qcol + k) * kPitch + sc];
            emit4<Cv>(dst + (long long)ly * S + qcol, min(4, tw - qcol), w, true);
          }
        }
      } else {
#pragma unroll 1
        for (int pass = 0; pass < kTile / 16; ++pass)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int ly = pass * 16 + wave * 4 + k;
            if (ly < th && lane < tw)
              dst[(long long)ly * S + lane] = Cv::apply(tile[(fx ? tw - 1 - lane : lane) * kPitch + (fy ? th - 1 - ly : ly)]);
          }
      }
      __syncthreads();  // the tile is filled again for the block's next plane
    } else if (out_quads) {
#pragma unroll 1
      for (int pass = 0; pass < kTile / 16; ++pass) {
        const int ly = pass * 16 + wave * 4 + qrow;
        if (ly < th && qcol < tw) {
          const int cnt = min(4, tw - qcol);
          unsigned w[4] = {0u, 0u, 0u, 0u};
          if (valid) {
            const int y = ty0 + ly, x = tx0 + qcol;
            const In* __restrict__ row = win + (long long)(fy ? S - 1 - y : y) * W;
            if (!fx) {
              fetch4(row + x, cnt, w);
            } else if (cnt == 4) {  // outputs x .. x + 3 are sources S-1-x down to S-4-x: one ascending access, registers swapped
              unsigned r[4];
              fetch4(row + (S - 4 - x), 4, r);
              w[0] = r[3], w[1] = r[2], w[2] = r[1], w[3] = r[0];
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (k < cnt) w[k] = word_of(row[S - 1 - x - k]);
            }
          }
          emit4<Cv>(dst + (long long)ly * S + qcol, cnt, w, valid);
        }
      }
    } else {
#pragma unroll 1
      for (int pass = 0; pass < kTile / 16; ++pass)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int ly = pass * 16 + wave * 4 + k;
          if (ly < th && lane < tw) {
            const int y = ty0 + ly, x = tx0 + lane;
            dst[(long long)ly * S + lane] =
                valid ? Cv::apply(word_of(win[(long long)(fy ? S - 1 - y : y) * W + (fx ? S - 1 - x : x)])) : Out(0);
          }
        }
    }
  }
}

// tiles along x and y, the (item, band) planes along z (at most 65535, the rest by the kernel's stride)
inline dim3 crop_grid(int S, long long planes) {
  const unsigned t = (unsigned)((S + kTile - 1) / kTile);
  return dim3(t, t, (unsigned)(planes > 65535 ? 65535 : planes));
}

inline int crop_check(const char* what, bool pointers, int n, int64_t L, int C, int C2, int H, int W, int S) {
  DRS_REQUIRE(pointers, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(n >= 1 && L >= 1 && C >= 1 && C2 >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= H && S <= W, DRS_ERR_SHAPE,
              "%s: n=%d L=%lld bands=%d/%d H=%d W=%d S=%d (need n, L, bands >= 1 and 1 <= S <= H, W)", what, n, (long long)L, C,
              C2, H, W, S);
  DRS_REQUIRE((S + kTile - 1) / kTile <= 65535, DRS_ERR_SHAPE, "%s: S=%d is more than 65535 tiles on a side", what, S);
  return DRS_OK;
}
}  // namespace

extern "C" int drs_crop_d4_u8(const uint8_t* cache_u8, const int32_t* items, int n, int64_t L, int C, int H, int W, int S,
                              uint8_t* out, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int st = crop_check("crop_d4_u8", cache_u8 && items && out, n, L, C, 1, H, W, S);
  if (st != DRS_OK) return st;
  DRS_LAUNCH(crop_d4_kernel<CopyU8>, crop_grid(S, (long long)n * C), dim3(kThreads), 0, s, Side<CopyU8>{cache_u8, out, C},
             Side<CopyU8>{nullptr, nullptr, 0}, (const int*)items, n, (long long)L, H, W, S, (const long long*)nullptr,
             (long long*)nullptr);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_crop_d4_u8_f32(const uint8_t* cache_u8, const int64_t* labels, const int32_t* items, int n, int64_t L, int C,
                                  int H, int W, int S, float* img_out, int64_t* labels_out, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int st = crop_check("crop_d4_u8_f32", cache_u8 && labels && items && img_out && labels_out, n, L, C, 1, H, W, S);
  if (st != DRS_OK) return st;
  DRS_LAUNCH(crop_d4_kernel<UnitU8>, crop_grid(S, (long long)n * C), dim3(kThreads), 0, s, Side<UnitU8>{cache_u8, img_out, C},
             Side<UnitU8>{nullptr, nullptr, 0}, (const int*)items, n, (long long)L, H, W, S, (const long long*)labels,
             (long long*)labels_out);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_crop_d4_pairs_f32(const float* sar_cache, const float* ndvi_cache, const int32_t* items, int n, int64_t L,
                                     int Cs, int Cn, int H, int W, int S, float* sar_out, float* ndvi_out, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int st = crop_check("crop_d4_pairs_f32", sar_cache && ndvi_cache && items && sar_out && ndvi_out, n, L, Cs, Cn, H, W, S);
  if (st != DRS_OK) return st;
  DRS_LAUNCH(crop_d4_kernel<UnitPm1>, crop_grid(S, (long long)n * (Cs + Cn)), dim3(kThreads), 0, s,
             Side<UnitPm1>{sar_cache, sar_out, Cs}, Side<UnitPm1>{ndvi_cache, ndvi_out, Cn}, (const int*)items, n, (long long)L,
             H, W, S, (const long long*)nullptr, (long long*)nullptr);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
