// apg_scan_spread.hip — k_scan_spread: the scan spread of a particle belief per candidate action (gfx950).  The
// definition, step by step, is the comment of apg_lidar_scan_spread in include/apgym_capi.h; this file restates only
// what the work split adds.  A sibling of k_scan_poses (apg_scan_poses.hip): the same staging of a packed map in LDS
// and the same per-ray code around apg::lidar_scan, copied rather than shared so that the measured kernel stays as it
// is -- but no scan value is written to memory: every reading becomes an integer and goes into integer sums.
//
// Determinism.  A reading enters the result only as v = rint(4096 s) and a weight only as q = rint(2^24 w).  S0, S1_b,
// S2_b and N are exact integer sums (uint64, int64, uint64, unsigned __int128), so neither the order in which the
// lanes add nor the work split can change a bit of them; what follows them is a fixed handful of f64 operations.
//
// Work assignment.  An ITEM is one (set i, candidate c) pair: K hypotheses, B beams.  A 256-thread workgroup takes a
// CONTIGUOUS run of items, so the candidates of one i that follow each other reuse the staged map, and walks an item
// in tiles of ppt = max(1, 256 / B) whole poses, rays numbered beam-minor (pose = r / B, beam = r % B) as in
// k_scan_poses.  Ray slot r of a tile (r < max(256, B)) is always walked by thread r % 256, and for B <= 256 its beam
// r % B is the same in every tile: the slot's partial sums of q v and q v^2 live in LDS, touched by their one thread
// only (so do the sums of q per pose slot, with the thread of its beam 0), with no barrier inside the walk over K.
// After the walk (one barrier) thread b adds the pose slots' q into S0 and beam b's ppt ray slots, forms
// N_b, and the workgroup reduces N; thread 0 writes the spread.  A set is never split across workgroups: no
// workspace, no second launch -- and M * A below the CU count leaves CUs idle.  A hypothesis of weight 0 is not
// scanned (it adds 0 to every sum).
//
// What reaches the walk is bounded as in k_scan_poses: finite poses, directions within 60 cells, poses further than 64
// cells outside the map read scan_empty.  LDS: the map <= 32 704 B + 16 B per ray slot (<= 16 384 B) + 8 B per pose
// slot (2 048 B) + 64 B.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/apgym_capi.h"
#include "apg_host.hpp"
#include "apg_rows_lds.hpp"
#include "apg_scan.hpp"

namespace apg {
namespace {

// (mirrored as SCAN_SPREAD_* in ap_gym_amd/_native.py: the tests place their shapes at these boundaries)
constexpr int SS_TILE = 256;             // threads per workgroup = rays per pass
constexpr int SS_MAX_K = 4096;           // hypotheses per set (S0 <= 2^36)
constexpr int SS_MAX_BEAMS = 1024;       // beams (LDS: 16 bytes of sums per beam)
constexpr int SS_MAX_GRID = 8192;        // workgroups per launch; each takes a contiguous run of items
constexpr float SS_POSE_MARGIN = 64.0f;  // poses further outside the map than this are not walked
constexpr float SS_MAX_DIR = 60.0f;      // |direction component| bound (the 64-column scan window)
#ifndef SS_MIN_WAVES
// Waves per SIMD the register budget is held to: k_scan_poses' measured choice (SP_MIN_WAVES) for the same
// walk; the two 64-bit multiply-adds per ray add no live state across it.
#define SS_MIN_WAVES 5
#endif

typedef unsigned __int128 u128;

struct ScanSpreadArgs {
  const uint64_t *occ;
  const int64_t *map_ids;
  const float *poses, *dirs, *weight;
  float *spread, *mean;
  uint32_t *err;
  int64_t n_src, m, items, per;  // items = m * a; per: items per workgroup
  int32_t h, w, a, k, beams, ppt;
  float range;
};

__global__ __launch_bounds__(SS_TILE, SS_MIN_WAVES) void k_scan_spread(ScanSpreadArgs A) {
  extern __shared__ uint64_t s_mem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = A.h, w = A.w, wpr = (w + 63) >> 6, words = h * wpr, B = A.beams, K = A.k;
  const int slots = max(SS_TILE, B);
  uint64_t *s_rows = s_mem;                                        // [h][wpr]
  uint64_t *s_s2 = s_mem + words;                                  // [slots] sum of q v^2 of ray slot r
  int64_t *s_s1 = reinterpret_cast<int64_t *>(s_s2 + slots);       // [slots] sum of q v
  uint64_t *s_s0 = reinterpret_cast<uint64_t *>(s_s1 + slots);     // [SS_TILE] sum of q of pose slot s (< ppt)
  uint64_t *s_red = s_s0 + SS_TILE;                                // [2][4] per wave: N low, N high
  const uint64_t last_mask = (w & 63) ? (1ULL << (w & 63)) - 1ULL : ~0ULL;
  const double inv_range = 1.0 / (double)A.range;
  const float xmax = (float)w + SS_POSE_MARGIN, ymax = (float)h + SS_POSE_MARGIN;
  const float nanv = __builtin_nanf("");
  uint32_t errbits = 0;
  int64_t staged = -1;
  const int64_t it0 = (int64_t)blockIdx.x * A.per, it1 = min(A.items, it0 + A.per);
  for (int64_t it = it0; it < it1; it++) {  // (uniform: every lane meets every barrier)
    const int64_t i = it / A.a;
    if (i != staged) {  // the set's map into LDS (every lane is past the previous item's walk: its second barrier)
      const int64_t id = A.map_ids ? A.map_ids[i] : (A.n_src == 1 ? 0 : i);
      const bool ok = id >= 0 && id < A.n_src;
      if (!ok && tid == 0) errbits |= APG_ERR_INDEX;
      for (int wi = tid; wi < words; wi += SS_TILE) {
        uint64_t v = ok ? A.occ[(size_t)id * words + wi] : 0ULL;
        if (wi % wpr == wpr - 1) v &= last_mask;
        s_rows[wi] = v;
      }
      staged = i;
      __syncthreads();
    }
    for (int r = tid; r < slots; r += SS_TILE) {  // (a thread's own slots: it walks ray slot r of every tile)
      s_s1[r] = 0;
      s_s2[r] = 0;
      if (r % B == 0 && r / B < SS_TILE) s_s0[r / B] = 0;  // (beam 0 of pose slot r / B)
    }
    const size_t pose0 = (size_t)it * K;  // poses [m][a][k][2]
    const float *wrow = A.weight ? A.weight + (size_t)i * K : nullptr;
    for (int k0 = 0; k0 < K; k0 += A.ppt) {
      const int nrays = min(A.ppt, K - k0) * B;  // <= slots
      for (int r = tid; r < nrays; r += SS_TILE) {
        const int s = r / B, b = r - s * B;
        const float px = A.poses[2 * (pose0 + k0 + s)], py = A.poses[2 * (pose0 + k0 + s) + 1];
        uint32_t q = 1u << 24;
        if (wrow) {
          const float wt = wrow[k0 + s];
          if (wt >= 0.0f && wt <= 1.0f) {  // (false for a NaN)
            q = (uint32_t)rintf(__fmul_rn(wt, 16777216.0f));
          } else {
            q = 0;
            errbits |= APG_ERR_BAD_POSE;
          }
        }
        if (!(fabsf(px) <= 3.4028235e38f && fabsf(py) <= 3.4028235e38f)) {
          q = 0;
          errbits |= APG_ERR_BAD_POSE;
        }
        if (b == 0) s_s0[s] += q;
        const float dx = A.dirs[2 * b], dy = A.dirs[2 * b + 1];
        if (!(fabsf(dx) <= SS_MAX_DIR && fabsf(dy) <= SS_MAX_DIR)) {  // the beam reads v = 0 for every pose
          errbits |= APG_ERR_BAD_POSE;
          continue;
        }
        if (q == 0) continue;
        const float qx = __fadd_rn(px, dx), qy = __fadd_rn(py, dy);
        const bool close_by = px >= -SS_POSE_MARGIN && px <= xmax && py >= -SS_POSE_MARGIN && py <= ymax;
        ScanOut o;
        if (close_by) {
          const RowsLds rows{s_rows, h, wpr, (int)floorf(fminf(px, qx)) - 1};
          o = lidar_scan(rows, px, py, qx, qy);
        } else {
          o = scan_empty(px, py, qx, qy);
        }
        const float nv = fminf(fmaxf(f32_div_inv(o.dist, inv_range), -1.0f), 1.0f);
        const int32_t v = (int32_t)rintf(__fmul_rn(nv, 4096.0f));  // |v| <= 4096
        s_s1[r] += (int64_t)q * v;
        s_s2[r] += (uint64_t)q * (uint64_t)(v * v);
      }
    }
    __syncthreads();  // every slot's sums are in LDS
    const int per_beam = B <= SS_TILE ? min(A.ppt, K) : 1;  // slots that hold sums of one beam, B apart
    uint64_t S0 = 0;
    if (tid < B)  // (the lanes that own a beam; thread 0 is one of them)
      for (int s = 0; s < per_beam; s++) S0 += s_s0[s];
    const double S0d = (double)S0;  // exact: S0 <= 2^36
    const bool has_beams = wave * 64 < B;  // (uniform in a wave) the other waves hold N = 0
    u128 n = 0;
    for (int b = tid; b < B; b += SS_TILE) {
      int64_t S1 = 0;
      uint64_t S2 = 0;
      for (int s = 0; s < per_beam; s++) {
        S1 += s_s1[s * B + b];
        S2 += s_s2[s * B + b];
      }
      const uint64_t a1 = (uint64_t)(S1 < 0 ? -S1 : S1);  // <= 2^48
      n += (u128)S0 * S2 - (u128)a1 * a1;                  // >= 0 (Cauchy-Schwarz); both products <= 2^96
      if (A.mean)
        A.mean[(size_t)it * B + b] = S0 ? (float)__dmul_rn(__ddiv_rn((double)S1, S0d), 0x1p-12) : nanv;
    }
    if (A.spread && has_beams) {
      uint64_t lo = (uint64_t)n, hi = (uint64_t)(n >> 64);
      for (int o = 32; o > 0; o >>= 1) {
        const u128 other = ((u128)__shfl_xor(hi, o, 64) << 64) | __shfl_xor(lo, o, 64);
        n += other;
        lo = (uint64_t)n;
        hi = (uint64_t)(n >> 64);
      }
      if (lane == 0) {
        s_red[wave] = lo;
        s_red[4 + wave] = hi;
      }
    }
    __syncthreads();  // the slots are read (the next item may clear them); the waves' N are in LDS
    if (A.spread && tid == 0) {
      u128 N = 0;
      for (int wv = 0; wv < 4 && wv * 64 < B; wv++) N += ((u128)s_red[4 + wv] << 64) | s_red[wv];
      A.spread[it] = S0 ? (float)__dmul_rn(__ddiv_rn((double)N, __dmul_rn(S0d, S0d)), 0x1p-24) : nanv;
    }
    // (no barrier here: the next item writes s_red after its own first barrier, which thread 0 reaches after the
    // reads above, and the slots were read before the barrier above)
  }
  if (errbits && A.err) atomicOr(A.err, errbits);
}

}  // namespace
}  // namespace apg

extern "C" int apg_lidar_scan_spread(const apg_scan_spread_args *a, apg_stream_t stream) {
  using namespace apg;
  if (!a) return fail(APG_E_INVALID, "scan_spread: null arguments");
  if (a->height < 1 || a->height > 511 || a->width < 1 || a->width > 511)
    return fail(APG_E_INVALID, "scan_spread: height and width must be in 1..511");
  if (a->beams < 1 || a->beams > SS_MAX_BEAMS) return fail(APG_E_INVALID, "scan_spread: beams must be in 1..1024");
  if (a->k < 1 || a->k > SS_MAX_K) return fail(APG_E_INVALID, "scan_spread: k must be in 1..4096");
  if (a->a < 1) return fail(APG_E_INVALID, "scan_spread: a must be >= 1");
  if (!(a->lidar_range > 0.0f) || a->lidar_range > 60.0f)
    return fail(APG_E_INVALID, "scan_spread: lidar_range must be in (0, 60] (64-column scan windows)");
  if (a->m < 0 || a->n_src < 0) return fail(APG_E_INVALID, "scan_spread: m and n_src must be >= 0");
  if (!a->spread && !a->mean) return fail(APG_E_INVALID, "scan_spread: neither spread nor mean is asked for");
  if (a->m == 0) return APG_OK;
  if (!a->poses || !a->beam_dirs || (!a->occ && a->n_src > 0))
    return fail(APG_E_INVALID, "scan_spread: null occ / poses / beam_dirs");
  if (!a->map_ids && a->n_src != 1 && a->m > a->n_src)
    return fail(APG_E_INVALID, "scan_spread: without map_ids, occ must hold one map or a map per set");
  const int words = a->height * ((a->width + 63) >> 6);
  ScanSpreadArgs A;
  A.occ = a->occ;
  A.map_ids = a->map_ids;
  A.poses = a->poses;
  A.dirs = a->beam_dirs;
  A.weight = a->weight;
  A.spread = a->spread;
  A.mean = a->mean;
  A.err = a->err;
  A.n_src = a->n_src;
  A.m = a->m;
  A.h = a->height;
  A.w = a->width;
  A.a = a->a;
  A.k = a->k;
  A.beams = a->beams;
  A.range = a->lidar_range;
  A.ppt = std::max(1, SS_TILE / a->beams);
  A.items = a->m * (int64_t)a->a;
  const int64_t grid = std::min<int64_t>(A.items, SS_MAX_GRID);
  A.per = (A.items + grid - 1) / grid;
  // <= 32 704 (map) + 16 384 (ray slots) + 2 048 (pose slots) + 64 (reduction) bytes
  const size_t lds = (size_t)words * 8 + (size_t)std::max(SS_TILE, (int)a->beams) * 16 + SS_TILE * 8 + 64;
  hipLaunchKernelGGL(k_scan_spread, dim3((unsigned)((A.items + A.per - 1) / A.per)), dim3(SS_TILE), lds,
                     (hipStream_t)stream, A);
  return check_launch("k_scan_spread");
}
