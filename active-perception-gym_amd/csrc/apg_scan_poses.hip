// apg_scan_poses.hip — k_scan_poses: exact LIDAR scans, and their fused scores, at caller-chosen poses (gfx950).
//
// For each pose set m of M: K poses, one packed map (map_ids[m] of an apg_lidar_state.occ-layout batch) and B beam
// directions.  Beam b of pose p is the segment p -> p + dir[b] (one f32 add per coordinate, as the step kernel and
// the reference's __get_obs build it), scanned with apg::lidar_scan of apg_scan.hpp unchanged -- the scan the env's
// observation is made of, bit for bit -- through the row source RowsLds (apg_rows_lds.hpp).  Outputs (either may be
// absent): scan[M][K][B] (normalised like the observation, or the distance in cells) and score[M][K], the squared error of the
// pose's normalised scan against observed[M][B], accumulated in f32 in beam order.
//
// Work assignment.  A ray is (pose, beam); rays are numbered beam-minor (pose = r / B, beam = r % B), so a wave's
// stores to `scan` are contiguous and its lanes walk neighbouring rows of one map.  A 256-thread workgroup works on
// one ITEM at a time:
//   * K * B <= 128 (small sets): `mpw` consecutive pose sets, all their rays at once (mpw * K * B <= 256, mpw <= 32,
//     mpw maps <= 32 KB of LDS), as k_unpack_maps batches small maps;
//   * otherwise one set's tile of ppt = max(1, 256 / B) whole poses: 256 rays or fewer per pass, and B > 256 is one
//     pose whose beams take several passes.
// An item's maps are staged in LDS once, with the padding bits at x >= width cleared (map_bits.py leaves them
// unspecified; read as they are they would be walls), and an id outside [0, n_src) staged as an all-zero map.  The
// grid is capped at SP_MAX_GRID workgroups; each takes a CONTIGUOUS run of items, so the tiles of one map that follow
// each other in a workgroup reuse the staged rows (M = 1 with a million poses stages its map once per workgroup).
// Scores: the tile's normalised values stay in LDS and one lane per pose adds them up in beam order.
//
// Inputs that must not reach the walk (a walk over saturated integer coordinates has no bound): a pose with a
// non-finite coordinate, or a direction with a non-finite component or one beyond 60 cells, is never scanned (NaN
// values, APG_ERR_BAD_POSE); a finite pose outside [-64, W + 64] x [-64, H + 64] reaches no map cell and reads
// scan_empty for every beam.  What is walked has |coordinates| < 640 and at most 124 crossings.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/apgym_capi.h"
#include "apg_host.hpp"
#include "apg_rows_lds.hpp"
#include "apg_scan.hpp"

namespace apg {
namespace {

// (mirrored as SCAN_POSES_* in ap_gym_amd/_native.py: the tests place their shapes at these boundaries)
constexpr int SP_TILE = 256;             // threads per workgroup = rays per pass
constexpr int SP_MAX_MPW = 32;           // pose sets per item (small sets)
constexpr int SP_MAX_GRID = 8192;        // 8 resident workgroups per CU, 4 rounds of them
constexpr int SP_MPW_MAP_BYTES = 32768;  // LDS the maps of one item may take (one 511 x 511 map: 32 704)
constexpr float SP_POSE_MARGIN = 64.0f;  // poses further outside the map than this are not walked
constexpr float SP_MAX_DIR = 60.0f;      // |direction component| bound (the 64-column scan window)
#ifndef SP_MIN_WAVES
// Waves per SIMD the register budget is held to.  The kernel is latency-bound (dependent LDS row reads and f64
// chains of the walk), so residency pays until the spills cost more: 3 waves (134 VGPRs, the compiler's own choice)
// 1 156 us, 4 (128) 1 007, 5 (96 VGPRs, 116 B of scratch) 940, 6 (80, 192 B) 1 037, 8 (64, 252 B) 1 115 us for
// 33.5 M rays (profiles/scan_poses_ab_waves.jsonl).
#define SP_MIN_WAVES 5
#endif

struct ScanPosesArgs {
  const uint64_t *occ;
  const int64_t *map_ids;
  const float *poses, *dirs, *observed;
  float *scan, *score;
  uint32_t *err;
  int64_t n_src, m, items, per;  // per: items per workgroup
  int32_t h, w, k, beams, normalize;
  int32_t mpw, ppt, tps;  // sets per item, poses per tile, tiles per set (1 when mpw > 1)
  float range;
};

__global__ __launch_bounds__(SP_TILE, SP_MIN_WAVES) void k_scan_poses(ScanPosesArgs A) {
  extern __shared__ uint64_t s_mem[];
  const int tid = threadIdx.x, h = A.h, w = A.w, wpr = (w + 63) >> 6, words = h * wpr, B = A.beams, K = A.k;
  uint64_t *s_rows = s_mem;                                               // [mpw][h][wpr]
  float *s_val = reinterpret_cast<float *>(s_mem + (size_t)A.mpw * words);  // [max(SP_TILE, B)] normalised values
  float *s_obs = s_val + max(SP_TILE, B);                                 // [SP_TILE] observed rows (B <= SP_TILE)
  const uint64_t last_mask = (w & 63) ? (1ULL << (w & 63)) - 1ULL : ~0ULL;
  const double inv_range = 1.0 / (double)A.range;
  const float xmax = (float)w + SP_POSE_MARGIN, ymax = (float)h + SP_POSE_MARGIN;
  const bool many = A.mpw > 1, obs_staged = A.score != nullptr && B <= SP_TILE;
  uint32_t errbits = 0;
  int64_t staged = -1;
  const int64_t it0 = (int64_t)blockIdx.x * A.per, it1 = min(A.items, it0 + A.per);
  for (int64_t it = it0; it < it1; it++) {
    const int64_t g = it / A.tps;
    const int t = (int)(it - g * A.tps);
    const int64_t m0 = g * A.mpw;
    const int nsets = (int)min((int64_t)A.mpw, A.m - m0);
    if (g != staged) {  // (uniform) the item's maps, and its observed rows, into LDS
      for (int i = tid; i < nsets * words; i += SP_TILE) {
        const int j = i / words, wi = i - j * words;
        const int64_t id = A.map_ids ? A.map_ids[m0 + j] : (A.n_src == 1 ? 0 : m0 + j);
        const bool ok = id >= 0 && id < A.n_src;
        if (!ok && wi == 0) errbits |= APG_ERR_INDEX;
        uint64_t v = ok ? A.occ[(size_t)id * words + wi] : 0ULL;
        if (wi % wpr == wpr - 1) v &= last_mask;
        s_rows[i] = v;
      }
      if (obs_staged)
        for (int i = tid; i < nsets * B; i += SP_TILE) s_obs[i] = A.observed[(size_t)m0 * B + i];
      staged = g;
      __syncthreads();
    }
    // slots = the item's poses, consecutive in `poses`: every pose of its nsets sets, or ppt poses of one set from k0
    const int k0 = many ? 0 : t * A.ppt;
    const int nslots = many ? nsets * K : min(A.ppt, K - k0);
    const int nrays = nslots * B;  // <= max(SP_TILE, B)
    const size_t pose0 = (size_t)m0 * K + k0;
    for (int r = tid; r < nrays; r += SP_TILE) {
      const int s = r / B, b = r - s * B;
      const int j = many ? s / K : 0;
      const float px = A.poses[2 * (pose0 + s)], py = A.poses[2 * (pose0 + s) + 1];
      const float dx = A.dirs[2 * b], dy = A.dirs[2 * b + 1];
      // (comparisons with a NaN are false: non-finite values fail both tests)
      const bool finite = fabsf(px) <= 3.4028235e38f && fabsf(py) <= 3.4028235e38f;
      const bool dir_ok = fabsf(dx) <= SP_MAX_DIR && fabsf(dy) <= SP_MAX_DIR;
      float d, nv;
      if (!finite || !dir_ok) {
        d = nv = __builtin_nanf("");
        errbits |= APG_ERR_BAD_POSE;
      } else {
        const float qx = __fadd_rn(px, dx), qy = __fadd_rn(py, dy);
        const bool close_by = px >= -SP_POSE_MARGIN && px <= xmax && py >= -SP_POSE_MARGIN && py <= ymax;
        ScanOut o;
        if (close_by) {
          const RowsLds rows{s_rows + j * words, h, wpr, (int)floorf(fminf(px, qx)) - 1};
          o = lidar_scan(rows, px, py, qx, qy);
        } else {
          o = scan_empty(px, py, qx, qy);
        }
        d = o.dist;
        nv = fminf(fmaxf(f32_div_inv(d, inv_range), -1.0f), 1.0f);
      }
      if (A.scan) A.scan[pose0 * B + r] = A.normalize ? nv : d;
      if (A.score) s_val[r] = nv;
    }
    if (A.score) {
      __syncthreads();
      if (tid < nslots) {  // (nslots <= SP_TILE) one lane per pose, in beam order
        const float *v = s_val + tid * B;
        float acc = 0.0f;
        if (obs_staged) {
          const float *o = s_obs + (many ? tid / K : 0) * B;
          for (int b = 0; b < B; b++) {
            const float e = __fsub_rn(v[b], o[b]);
            acc = __fadd_rn(acc, __fmul_rn(e, e));
          }
        } else {
          const float *o = A.observed + (size_t)m0 * B;
          for (int b = 0; b < B; b++) {
            const float e = __fsub_rn(v[b], o[b]);
            acc = __fadd_rn(acc, __fmul_rn(e, e));
          }
        }
        A.score[pose0 + tid] = acc;
      }
    }
    __syncthreads();  // the next item overwrites s_val, and s_rows / s_obs when its maps differ
  }
  if (errbits && A.err) atomicOr(A.err, errbits);
}

}  // namespace
}  // namespace apg

extern "C" int apg_lidar_scan_poses(const apg_scan_poses_args *a, apg_stream_t stream) {
  using namespace apg;
  if (!a) return fail(APG_E_INVALID, "scan_poses: null arguments");
  if (a->height < 1 || a->height > 511 || a->width < 1 || a->width > 511)
    return fail(APG_E_INVALID, "scan_poses: height and width must be in 1..511");
  if (a->beams < 1 || a->beams > 4096) return fail(APG_E_INVALID, "scan_poses: beams must be in [1, 4096]");
  if (!(a->lidar_range > 0.0f) || a->lidar_range > 60.0f)
    return fail(APG_E_INVALID, "scan_poses: lidar_range must be in (0, 60] (64-column scan windows)");
  if (a->m < 0 || a->k < 0 || a->n_src < 0) return fail(APG_E_INVALID, "scan_poses: m, k and n_src must be >= 0");
  if (a->m == 0 || a->k == 0) return APG_OK;
  if (!a->poses || !a->beam_dirs || (!a->occ && a->n_src > 0))
    return fail(APG_E_INVALID, "scan_poses: null occ / poses / beam_dirs");
  if (!a->scan && !a->score) return fail(APG_E_INVALID, "scan_poses: neither scan nor score is asked for");
  if (a->score && !a->observed) return fail(APG_E_INVALID, "scan_poses: score needs observed");
  if (!a->map_ids && a->n_src != 1 && a->m > a->n_src)
    return fail(APG_E_INVALID, "scan_poses: without map_ids, occ must hold one map or a map per pose set");
  const int words = a->height * ((a->width + 63) >> 6);
  ScanPosesArgs A;
  A.occ = a->occ;
  A.map_ids = a->map_ids;
  A.poses = a->poses;
  A.dirs = a->beam_dirs;
  A.observed = a->observed;
  A.scan = a->scan;
  A.score = a->score;
  A.err = a->err;
  A.n_src = a->n_src;
  A.m = a->m;
  A.h = a->height;
  A.w = a->width;
  A.k = a->k;
  A.beams = a->beams;
  A.normalize = a->normalize;
  A.range = a->lidar_range;
  const int64_t set_rays = (int64_t)a->k * a->beams;
  int64_t mpw = 1;
  if (2 * set_rays <= SP_TILE)
    mpw = std::max<int64_t>(1, std::min<int64_t>({SP_MAX_MPW, SP_TILE / set_rays, SP_MPW_MAP_BYTES / (8 * words), a->m}));
  A.mpw = (int32_t)mpw;
  A.ppt = std::max(1, SP_TILE / a->beams);
  A.tps = mpw > 1 ? 1 : (a->k + A.ppt - 1) / A.ppt;
  A.items = (a->m + mpw - 1) / mpw * A.tps;
  const int64_t grid = std::min<int64_t>(A.items, SP_MAX_GRID);
  A.per = (A.items + grid - 1) / grid;
  // <= 32 704 (maps) + 16 384 (values) + 1 024 (observed) bytes
  const size_t lds = (size_t)mpw * words * 8 + ((size_t)std::max(SP_TILE, (int)a->beams) + SP_TILE) * sizeof(float);
  hipLaunchKernelGGL(k_scan_poses, dim3((unsigned)((A.items + A.per - 1) / A.per)), dim3(SP_TILE), lds,
                     (hipStream_t)stream, A);
  return check_launch("k_scan_poses");
}
