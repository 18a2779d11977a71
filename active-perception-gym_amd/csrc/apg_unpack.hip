// apg_unpack.hip — k_unpack_maps: occupancy bit rows -> dense maps of a chosen element type (gfx950).
//
// The LIDAR envs keep every env's current map as bit rows (apg_lidar_state.occ, u64 [N][H][ceil(W/64)], bit x & 63 of
// word x >> 6 of row y = cell (y, x), 1 = wall).  map_obs="bits" hands those rows out as the observation; this kernel
// expands a chosen subset of them to [count][H][W] maps of f32 / f16 / bf16 / u8 (apg_lidar_unpack_maps), e.g. the
// minibatch a learner draws from a replay buffer of bit rows.
//
// The kernel is HBM-write-bound (it reads H * wpr * 8 bytes and writes H * W * sizeof(T) per map), so it is built
// around the store: every lane's store is one aligned 16-byte vector (4 f32, 8 f16/bf16 or 16 u8 cells) and a wave
// instruction covers 1 KB of contiguous output.  As bitmap_map_obs (apg_maze.hpp) does for f32, a map's rows are first
// re-laid in LDS as ONE row-major bit string (bit c = cell c = y * W + x), so the cells of a 16-byte store are
// consecutive bits whatever W is; with W % 64 == 0 that string is the rows themselves and they are copied as they are.
// The padding bits at x >= W are masked off by the re-lay and never reach the output.  A map's output is cut into the
// 16-byte chunks of its ABSOLUTE address range: every chunk that lies wholly inside the map is one non-temporal vector
// store, the (at most two) partial chunks at its unaligned head and tail are element stores.
//
// Work assignment: a 256-thread workgroup takes a batch of `mpw` consecutive output maps per grid-stride iteration,
// mpw = 1 for large maps and up to 32 for small ones (so an iteration has up to 16 KB of stores in flight); inside a
// batch the threads form 256 / ts teams of ts threads (ts = the map's chunk count rounded up to a power of two,
// 8..256), one map per team at a time.  The grid is capped at 8 192 workgroups, so 65 536 maps are not 65 536 tiny workgroups;
// smaller batches and a larger grid measured faster than 32 KB batches on 2 048 workgroups.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/apgym_capi.h"
#include "apg_host.hpp"

namespace apg {
namespace {

constexpr int UNPACK_THREADS = 256;
constexpr int UNPACK_MAX_MPW = 32;         // maps per workgroup iteration (small maps)
constexpr int UNPACK_BATCH_BYTES = 16384;  // output bytes a workgroup iteration aims at
constexpr int UNPACK_MAX_GRID = 8192;      // 8 resident workgroups per CU, 4 rounds of them

// Words of a map's row-major bit string, + 1 zero word (a chunk's bits are read from two consecutive words).
__host__ __device__ inline int lin_words(int h, int w) { return (h * w + 63) / 64 + 1; }

struct UnpackArgs {
  const uint64_t *occ;
  const int64_t *env_ids;
  void *dst;
  uint32_t *err;
  int64_t n_src, count;
  int32_t h, w, mpw, ts;
  uint32_t wall;  // the wall value's bit pattern in the element type
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The 16 / ES elements of one chunk from their bits (bit i = element i): wall where set, 0 elsewhere.
template <int ES>
__device__ __forceinline__ u32x4 expand(uint32_t b, uint32_t wall) {
  u32x4 v;
  if constexpr (ES == 4) {
    v.x = (b & 1u) ? wall : 0u;
    v.y = (b & 2u) ? wall : 0u;
    v.z = (b & 4u) ? wall : 0u;
    v.w = (b & 8u) ? wall : 0u;
  } else if constexpr (ES == 2) {
    // bits 2i, 2i + 1 -> the halves of dword i (wall <= 0xffff: the products do not overlap)
    v.x = ((b & 1u) | ((b & 2u) << 15)) * wall;
    v.y = (((b >> 2) & 1u) | ((b & 8u) << 13)) * wall;
    v.z = (((b >> 4) & 1u) | ((b & 32u) << 11)) * wall;
    v.w = (((b >> 6) & 1u) | ((b & 128u) << 9)) * wall;
  } else {
    // a nibble's bits to the low bit of each byte of a dword: n * 0x00204081 = n | n << 7 | n << 14 | n << 21
    v.x = (((b & 15u) * 0x00204081u) & 0x01010101u) * wall;
    v.y = ((((b >> 4) & 15u) * 0x00204081u) & 0x01010101u) * wall;
    v.z = ((((b >> 8) & 15u) * 0x00204081u) & 0x01010101u) * wall;
    v.w = ((((b >> 12) & 15u) * 0x00204081u) & 0x01010101u) * wall;
  }
  return v;
}

template <int ES>
struct Elem;
template <>
struct Elem<4> {
  typedef uint32_t type;
};
template <>
struct Elem<2> {
  typedef uint16_t type;
};
template <>
struct Elem<1> {
  typedef uint8_t type;
};

template <int ES>
__global__ __launch_bounds__(UNPACK_THREADS) void k_unpack_maps(UnpackArgs A) {
  typedef typename Elem<ES>::type elem_t;
  constexpr int CPV = 16 / ES;  // cells per 16-byte chunk
  extern __shared__ uint64_t s_lin[];  // [mpw][lin_words]
  const int tid = threadIdx.x, h = A.h, w = A.w, wpr = (w + 63) >> 6;
  const int cells = h * w, nlin = lin_words(h, w), words = h * wpr;
  const int team = tid / A.ts, tl = tid & (A.ts - 1), teams = UNPACK_THREADS / A.ts;
  const int64_t nbatch = (A.count + A.mpw - 1) / A.mpw;
  const bool rows_are_lin = (w & 63) == 0;
  for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
    // ---- the batch's bit strings into LDS
    for (int j = team; j < A.mpw; j += teams) {
      const int64_t m = b * A.mpw + j;
      if (m >= A.count) break;
      const int64_t id = A.env_ids ? A.env_ids[m] : m;
      const bool ok = id >= 0 && id < A.n_src;
      if (!ok && tl == 0 && A.err) atomicOr(A.err, APG_ERR_INDEX);
      const uint64_t *rows = A.occ + (ok ? (size_t)id * words : 0);
      uint64_t *lin = s_lin + j * nlin;
      for (int i = tl; i < nlin; i += A.ts) {
        uint64_t v = 0;
        const int c = 64 * i;
        if (ok && c < cells) {
          if (rows_are_lin) {
            v = rows[i];
          } else {
            int y = c / w, x = c - y * w, filled = 0;
            while (filled < 64 && y < h) {
              const int k = min(64 - filled, w - x);  // bits [x, x + k) of row y
              const uint64_t *r = rows + y * wpr;
              const int q = x >> 6, o = x & 63;
              const uint64_t lo = r[q], hi = (o + k > 64) ? r[q + 1] : 0ULL;  // (o + k > 64 only where q + 1 < wpr)
              uint64_t bits = (lo >> o) | ((hi << 1) << (63 - o));
              if (k < 64) bits &= (1ULL << k) - 1ULL;
              v |= bits << filled;
              filled += k;
              x = 0;
              y++;
            }
          }
        }
        lin[i] = v;
      }
    }
    __syncthreads();
    // ---- the batch's maps out: the 16-byte chunks of each map's absolute address range
    for (int j = team; j < A.mpw; j += teams) {
      const int64_t m = b * A.mpw + j;
      if (m >= A.count) break;
      const uint64_t *lin = s_lin + j * nlin;
      elem_t *dst = reinterpret_cast<elem_t *>(A.dst) + (size_t)m * cells;
      const int head = (int)((uintptr_t)dst & 15u) / ES;  // elements of the first chunk that precede the map
      const int nchunk = (head + cells + CPV - 1) / CPV;
      for (int k = tl; k < nchunk; k += A.ts) {
        const int c0 = k * CPV - head;  // the chunk's first cell (< 0: the chunk begins before the map)
        if (c0 >= 0 && c0 + CPV <= cells) {
          const int wi = c0 >> 6;
          const uint32_t o = (uint32_t)c0 & 63u;
          const uint32_t bits = (uint32_t)((lin[wi] >> o) | ((lin[wi + 1] << 1) << (63u - o)));
          __builtin_nontemporal_store(expand<ES>(bits, A.wall), reinterpret_cast<u32x4 *>(dst + c0));
        } else {
          for (int c = max(c0, 0); c < min(c0 + CPV, cells); c++)
            dst[c] = ((lin[c >> 6] >> (c & 63)) & 1ULL) ? (elem_t)A.wall : (elem_t)0;
        }
      }
    }
    __syncthreads();  // the next batch overwrites s_lin
  }
}

uint32_t float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  return u;
}

// float32 -> float16 bits, round-to-nearest-even (subnormals through a float add whose ulp is the f16 subnormal step)
uint32_t f16_bits_rne(float f) {
  uint32_t u = float_bits(f);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  uint32_t o;
  if (u >= (143u << 23)) {  // >= 65536, inf, NaN
    o = u > (255u << 23) ? 0x7e00u : 0x7c00u;
  } else if (u < (113u << 23)) {  // below the smallest normal f16
    float t;
    memcpy(&t, &u, sizeof(t));
    t += 0.5f;
    o = float_bits(t) - (126u << 23);
  } else {
    const uint32_t odd = (u >> 13) & 1u;
    u += ((uint32_t)(15 - 127) << 23) + 0xfffu;
    u += odd;
    o = u >> 13;
  }
  return sign | o;
}

// float32 -> bfloat16 bits, round-to-nearest-even
uint32_t bf16_bits_rne(float f) {
  uint32_t u = float_bits(f);
  if ((u & 0x7fffffffu) > (255u << 23)) return (u >> 16) | 0x40u;  // NaN stays a (quiet) NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace
}  // namespace apg

extern "C" int apg_lidar_unpack_maps(const uint64_t *occ, int64_t n_src, int height, int width,
                                     const int64_t *env_ids, int64_t count, int dtype, float wall, void *dst,
                                     uint32_t *err, apg_stream_t stream) {
  using namespace apg;
  if (height < 1 || height > 511 || width < 1 || width > 511)
    return fail(APG_E_INVALID, "unpack_maps: height and width must be in 1..511");
  if (count < 0 || n_src < 0) return fail(APG_E_INVALID, "unpack_maps: count and n_src must be >= 0");
  int es;
  uint32_t wall_bits;
  switch (dtype) {
    case APG_UNPACK_F32: es = 4, wall_bits = float_bits(wall); break;
    case APG_UNPACK_F16: es = 2, wall_bits = f16_bits_rne(wall); break;
    case APG_UNPACK_BF16: es = 2, wall_bits = bf16_bits_rne(wall); break;
    case APG_UNPACK_U8:
      if (!(wall >= 0.0f && wall <= 255.0f) || wall != std::floor(wall))
        return fail(APG_E_INVALID, "unpack_maps: the wall value of u8 maps must be an integer in 0..255");
      es = 1, wall_bits = (uint32_t)wall;
      break;
    default: return fail(APG_E_INVALID, "unpack_maps: dtype must be one of APG_UNPACK_*");
  }
  if (count == 0) return APG_OK;
  if (!dst || (!occ && n_src > 0)) return fail(APG_E_INVALID, "unpack_maps: null occ / dst");
  if ((uintptr_t)dst % es) return fail(APG_E_INVALID, "unpack_maps: dst is not aligned to its element type");
  const int cells = height * width, cpv = 16 / es;
  UnpackArgs A;
  A.occ = occ;
  A.env_ids = env_ids;
  A.dst = dst;
  A.err = err;
  A.n_src = n_src;
  A.count = count;
  A.h = height;
  A.w = width;
  A.wall = wall_bits;
  // maps per iteration: a power of two, ~UNPACK_BATCH_BYTES of output; threads per map: its chunks, a power of two
  int mpw = 1;
  while (mpw < UNPACK_MAX_MPW && (int64_t)2 * mpw * cells * es <= UNPACK_BATCH_BYTES) mpw <<= 1;
  A.mpw = mpw;
  A.ts = std::min(UNPACK_THREADS, std::max(8, pow2_ceil((cells + cpv - 1) / cpv + 1)));
  const int64_t nbatch = (count + mpw - 1) / mpw;
  const unsigned grid = (unsigned)std::min<int64_t>(nbatch, UNPACK_MAX_GRID);
  const size_t lds = (size_t)mpw * lin_words(height, width) * sizeof(uint64_t);  // <= 33 KB (one 511 x 511 map)
  hipStream_t s = (hipStream_t)stream;
  if (es == 4)
    hipLaunchKernelGGL(k_unpack_maps<4>, dim3(grid), dim3(UNPACK_THREADS), lds, s, A);
  else if (es == 2)
    hipLaunchKernelGGL(k_unpack_maps<2>, dim3(grid), dim3(UNPACK_THREADS), lds, s, A);
  else
    hipLaunchKernelGGL(k_unpack_maps<1>, dim3(grid), dim3(UNPACK_THREADS), lds, s, A);
  return check_launch("k_unpack_maps");
}
