// apg_move_poses.hip — k_move_poses: exact open-loop rollouts of candidate actions from caller-chosen poses (gfx950).
//
// For each candidate set m of M: K start poses, K action sequences of T actions and one packed map (map_ids[m] of an
// apg_lidar_state.occ-layout batch).  One action applied to a pose is LIDARLocalization2DEnv's movement
// (ap_gym/envs/lidar_localization2d.py:330-375) in the float32 operation order of phase 1 of k_lidar_step
// (apg_lidar.hip, restated here: that file's include closure keys the committed profile tables and is not touched):
// base reward, clamp to unit length, one exact scan to the target, advance to the first wall, slide along the kept
// positive components of what remains (two axis scans, candidate 0 when its distance is > 0), the `left the map`
// test before the clip to [0, W] x [0, H].  A candidate terminates at the first action after which it has left the
// map or has used up max_steps[m] actions (TimeLimit with issue_termination=True); later entries repeat its final
// pose.  Every scan is apg::lidar_scan of apg_scan.hpp unchanged, through RowsLds (apg_rows_lds.hpp) with the
// window of k_scan_poses, x0 = floor(min(px, qx)) - 1.
//
// Work assignment.  One lane per candidate (m, k), looping over its T actions: the actions of a candidate depend on
// each other, the candidates do not.  A 256-thread workgroup works on one ITEM at a time, the scheme of k_scan_poses:
//   * 2 K <= 256 (small sets): `mpw` consecutive sets, all their candidates at once (mpw * K <= 256, mpw <= 32, mpw
//     maps <= 32 KB of LDS);
//   * otherwise one set's tile of 256 candidates.
// An item's maps are staged in LDS once, padding bits at x >= width cleared, an id outside [0, n_src) staged as an
// all-zero map.  The grid is capped at MP_MAX_GRID workgroups; each takes a CONTIGUOUS run of items, so consecutive
// tiles of one set reuse the staged map.
//
// The three scans of an action share ONE call site (a three-pass loop, not unrolled): lidar_scan inlines to several
// hundred instructions and its register demand sets the kernel's, and lanes that slide run their two slide scans
// together while the lanes that met no wall wait (divergence: only lanes that hit a wall have passes 1 and 2).
// Stores: a lane writes its 8-byte pose at stride 8 T; staging a tile's steps in LDS for row-contiguous stores was
// not tried (DESIGN 5.3 lists what was not measured).
//
// Inputs that must not reach the walk: a candidate with a non-finite start pose or action is never scanned from that
// action on (NaN outputs, APG_ERR_BAD_POSE); a scan that starts further than 64 cells outside the map reaches no cell
// and takes scan_empty.  Actions are clamped to length 1 and slides are no longer than what remains of them, so every
// walked segment is at most 1 cell long and has |coordinates| < 640.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/apgym_capi.h"
#include "apg_host.hpp"
#include "apg_rows_lds.hpp"
#include "apg_scan.hpp"

namespace apg {
namespace {

// (mirrored as MOVE_POSES_* in ap_gym_amd/_native.py: the tests place their shapes at these boundaries)
constexpr int MP_TILE = 256;             // threads per workgroup = candidates per item
constexpr int MP_MAX_MPW = 32;           // candidate sets per item (small sets)
constexpr int MP_MAX_GRID = 8192;        // 8 resident workgroups per CU, 4 rounds of them
constexpr int MP_MPW_MAP_BYTES = 32768;  // LDS the maps of one item may take (one 511 x 511 map: 32 704)
constexpr int MP_MAX_T = 4096;           // actions per candidate
constexpr float MP_POSE_MARGIN = 64.0f;  // scans that start further outside the map than this are not walked
#ifndef MP_MIN_WAVES
// Waves per SIMD the register budget is held to, by A/B (profiles/move_poses_ab_waves.jsonl): 3 waves
// (150 VGPRs, the compiler's own choice) 240 us, 4 (128 VGPRs, 64 B of scratch) 231-235, 5 (96, 172 B; k_scan_poses'
// choice for the same walk) 273-283, 6 (80, 268 B) 511, 8 (64, 328 B) 554-557 us for 4.2 M actions at T = 8.  The
// loop over T keeps more state live across the scan than k_scan_poses has, so the spills start to cost a wave earlier.
#define MP_MIN_WAVES 4
#endif

struct MovePosesArgs {
  const uint64_t *occ;
  const int64_t *map_ids;
  const float *poses, *actions, *origin;
  const int32_t *max_steps;
  const uint8_t *origin_alias;
  float *pos, *base_reward, *odometry;
  int32_t *steps;
  uint8_t *terminated;
  uint32_t *err;
  int64_t n_src, m, items, per;  // per: items per workgroup
  int32_t h, w, k, t;
  int32_t mpw, tps;  // sets per item, tiles per set (1 when mpw > 1)
};

APG_DEV bool finite2(float x, float y) {  // (comparisons with a NaN are false)
  return fabsf(x) <= 3.4028235e38f && fabsf(y) <= 3.4028235e38f;
}

__global__ __launch_bounds__(MP_TILE, MP_MIN_WAVES) void k_move_poses(MovePosesArgs A) {
  extern __shared__ uint64_t s_rows[];  // [mpw][h][wpr]
  const int tid = threadIdx.x, h = A.h, w = A.w, wpr = (w + 63) >> 6, words = h * wpr, K = A.k, T = A.t;
  const uint64_t last_mask = (w & 63) ? (1ULL << (w & 63)) - 1ULL : ~0ULL;
  const float mapw = (float)w, maph = (float)h;
  const float xmax = mapw + MP_POSE_MARGIN, ymax = maph + MP_POSE_MARGIN;
  const double inv_2w = 1.0 / (double)__fadd_rn(mapw, mapw), inv_2h = 1.0 / (double)__fadd_rn(maph, maph);
  const float nanv = __builtin_nanf("");
  const bool many = A.mpw > 1;
  uint32_t errbits = 0;
  int64_t staged = -1;
  const int64_t it0 = (int64_t)blockIdx.x * A.per, it1 = min(A.items, it0 + A.per);
  for (int64_t it = it0; it < it1; it++) {
    const int64_t g = it / A.tps;
    const int tile = (int)(it - g * A.tps);
    const int64_t m0 = g * A.mpw;
    const int nsets = (int)min((int64_t)A.mpw, A.m - m0);
    if (g != staged) {  // (uniform) the item's maps into LDS
      __syncthreads();  // every lane is done with the maps of the item before
      for (int i = tid; i < nsets * words; i += MP_TILE) {
        const int j = i / words, wi = i - j * words;
        const int64_t id = A.map_ids ? A.map_ids[m0 + j] : (A.n_src == 1 ? 0 : m0 + j);
        const bool ok = id >= 0 && id < A.n_src;
        if (!ok && wi == 0) errbits |= APG_ERR_INDEX;
        uint64_t v = ok ? A.occ[(size_t)id * words + wi] : 0ULL;
        if (wi % wpr == wpr - 1) v &= last_mask;
        s_rows[i] = v;
      }
      staged = g;
      __syncthreads();
    }
    // slots = the item's candidates, consecutive in `poses`: every one of its nsets sets, or 256 of one set from k0
    const int k0 = many ? 0 : tile * MP_TILE;
    const int nslots = many ? nsets * K : min(MP_TILE, K - k0);
    if (tid >= nslots) continue;  // (no barrier below this line inside the item)
    const int j = many ? tid / K : 0;
    const int64_t set = m0 + j;
    const size_t c = (size_t)m0 * K + k0 + tid;  // candidate index m * K + k
    const uint64_t *rows = s_rows + j * words;
    float px = A.poses[2 * c], py = A.poses[2 * c + 1];
    float ox = 0.0f, oy = 0.0f;
    bool alias = false;
    if (A.origin) {
      ox = A.origin[2 * set];
      oy = A.origin[2 * set + 1];
      alias = A.origin_alias && A.origin_alias[set] != 0;
    }
    const int limit = A.max_steps ? A.max_steps[set] : 0;
    const float *act = A.actions + 2 * c * T;
    float *o_pos = A.pos + 2 * c * T;
    float *o_br = A.base_reward ? A.base_reward + c * T : nullptr;
    float *o_odo = A.odometry ? A.odometry + 2 * c * T : nullptr;
    bool bad = !finite2(px, py), term = false;
    int steps = 0;
    float odx = 0.0f, ody = 0.0f;
    if (bad) px = py = odx = ody = nanv;
    for (int t = 0; t < T; t++) {
      float br = 0.0f;
      if (!bad && !term) {
        float ax = act[2 * t], ay = act[2 * t + 1];
        bad = !finite2(ax, ay);
        if (!bad) {
          br = __fsub_rn(0.1f, __fmul_rn(0.001f, __fadd_rn(__fmul_rn(ax, ax), __fmul_rn(ay, ay))));
          const float mag = norm_f32(ax, ay);
          if (mag > 1.0f) {
            ax = f32_div(ax, mag);
            ay = f32_div(ay, mag);
          }
          const float tx = __fadd_rn(px, ax), ty = __fadd_rn(py, ay);
          float dirx = __fsub_rn(tx, px), diry = __fsub_rn(ty, py);
          const float total = norm_f32(dirx, diry);
          // pass 0: the scan to the target; passes 1, 2 (lanes that slide): the two axis candidates eye(2) * kept
          float qx = tx, qy = ty, c0x = 0.0f, c1y = 0.0f, d0 = 0.0f, d1 = 0.0f;
          bool run = total > 0.0f;
#pragma clang loop unroll(disable)
          for (int pass = 0; pass < 3; pass++) {
            float d = 0.0f;
            if (run) {
              const bool close_by = px >= -MP_POSE_MARGIN && px <= xmax && py >= -MP_POSE_MARGIN && py <= ymax;
              if (close_by) {
                const RowsLds src{rows, h, wpr, (int)floorf(fminf(px, qx)) - 1};
                d = lidar_scan(src, px, py, qx, qy).dist;
              } else {
                d = scan_empty(px, py, qx, qy).dist;
              }
            }
            if (pass == 0) {
              bool slide = false;
              if (run) {
                dirx = f32_div(dirx, total);
                diry = f32_div(diry, total);
                px = __fadd_rn(px, __fmul_rn(dirx, d));
                py = __fadd_rn(py, __fmul_rn(diry, d));
                const float rem = __fsub_rn(total, d);
                if (rem > 1e-5f) {  // slide along the wall (:345-364)
                  const float rvx = __fmul_rn(dirx, rem), rvy = __fmul_rn(diry, rem);
                  const bool kx = rvx > 1e-5f, ky = rvy > 1e-5f;
                  slide = kx || ky;
                  c0x = kx ? rvx : rvy;  // with one kept component both candidates use it
                  c1y = ky ? rvy : rvx;
                }
              }
              run = slide;
              qx = __fadd_rn(px, c0x);
              qy = __fadd_rn(py, 0.0f);
            } else if (pass == 1) {
              d0 = d;
              qx = __fadd_rn(px, 0.0f);
              qy = __fadd_rn(py, c1y);
            } else {
              d1 = d;
            }
          }
          if (run) {
            float cx, cy, dd;
            if (d0 > 0.0f) {
              cx = c0x;
              cy = 0.0f;
              dd = d0;
            } else {
              cx = 0.0f;
              cy = c1y;
              dd = d1;
            }
            const float nrm = norm_f32(cx, cy);
            px = __fadd_rn(px, __fmul_rn(f32_div(cx, nrm), dd));
            py = __fadd_rn(py, __fmul_rn(f32_div(cy, nrm), dd));
          }
          if (alias && t == 0) {  // initial_pos aliases pos until np.clip rebinds it (:305, :371)
            ox = px;
            oy = py;
          }
          term = px < 0.0f || py < 0.0f || px >= mapw || py >= maph;
          px = fminf(fmaxf(px, 0.0f), mapw);
          py = fminf(fmaxf(py, 0.0f), maph);
          steps = t + 1;
          if (limit > 0 && steps >= limit) term = true;  // TimeLimit(issue_termination=True)
          // odometry (:263-270), as the step kernel writes it
          odx = __fsub_rn(__fmul_rn(f32_div_inv(__fadd_rn(__fsub_rn(px, ox), mapw), inv_2w), 2.0f), 1.0f);
          ody = __fsub_rn(__fmul_rn(f32_div_inv(__fadd_rn(__fsub_rn(py, oy), maph), inv_2h), 2.0f), 1.0f);
        }
        if (bad) {
          term = false;
          px = py = odx = ody = nanv;
        }
      }
      if (bad) br = nanv;
      o_pos[2 * t] = px;  // (two 4-byte stores: the C ABI asks for no more than float alignment)
      o_pos[2 * t + 1] = py;
      if (o_br) o_br[t] = br;
      if (o_odo) {
        o_odo[2 * t] = odx;
        o_odo[2 * t + 1] = ody;
      }
    }
    if (bad) errbits |= APG_ERR_BAD_POSE;
    A.steps[c] = steps;
    A.terminated[c] = term ? 1 : 0;
  }
  if (errbits && A.err) atomicOr(A.err, errbits);
}

}  // namespace
}  // namespace apg

extern "C" int apg_lidar_move_poses(const apg_move_poses_args *a, apg_stream_t stream) {
  using namespace apg;
  if (!a) return fail(APG_E_INVALID, "move_poses: null arguments");
  if (a->height < 1 || a->height > 511 || a->width < 1 || a->width > 511)
    return fail(APG_E_INVALID, "move_poses: height and width must be in 1..511");
  if (a->t < 1 || a->t > MP_MAX_T) return fail(APG_E_INVALID, "move_poses: t must be in [1, 4096]");
  if (a->m < 0 || a->k < 0 || a->n_src < 0) return fail(APG_E_INVALID, "move_poses: m, k and n_src must be >= 0");
  if (a->odometry && !a->origin) return fail(APG_E_INVALID, "move_poses: odometry needs origin");
  if (a->origin_alias && !a->origin) return fail(APG_E_INVALID, "move_poses: origin_alias needs origin");
  if (a->m == 0 || a->k == 0) return APG_OK;
  if (!a->poses || !a->actions || (!a->occ && a->n_src > 0))
    return fail(APG_E_INVALID, "move_poses: null occ / poses / actions");
  if (!a->pos || !a->steps || !a->terminated) return fail(APG_E_INVALID, "move_poses: null pos / steps / terminated");
  if (!a->map_ids && a->n_src != 1 && a->m > a->n_src)
    return fail(APG_E_INVALID, "move_poses: without map_ids, occ must hold one map or a map per candidate set");
  const int words = a->height * ((a->width + 63) >> 6);
  MovePosesArgs A;
  A.occ = a->occ;
  A.map_ids = a->map_ids;
  A.poses = a->poses;
  A.actions = a->actions;
  A.origin = a->origin;
  A.max_steps = a->max_steps;
  A.origin_alias = a->origin_alias;
  A.pos = a->pos;
  A.base_reward = a->base_reward;
  A.odometry = a->odometry;
  A.steps = a->steps;
  A.terminated = a->terminated;
  A.err = a->err;
  A.n_src = a->n_src;
  A.m = a->m;
  A.h = a->height;
  A.w = a->width;
  A.k = a->k;
  A.t = a->t;
  int64_t mpw = 1;
  if (2 * (int64_t)a->k <= MP_TILE)
    mpw = std::max<int64_t>(1, std::min<int64_t>({MP_MAX_MPW, MP_TILE / a->k, MP_MPW_MAP_BYTES / (8 * words), a->m}));
  A.mpw = (int32_t)mpw;
  A.tps = mpw > 1 ? 1 : (a->k + MP_TILE - 1) / MP_TILE;
  A.items = (a->m + mpw - 1) / mpw * A.tps;
  const int64_t grid = std::min<int64_t>(A.items, MP_MAX_GRID);
  A.per = (A.items + grid - 1) / grid;
  const size_t lds = (size_t)mpw * words * 8;  // <= 32 704 bytes
  hipLaunchKernelGGL(k_move_poses, dim3((unsigned)((A.items + A.per - 1) / A.per)), dim3(MP_TILE), lds,
                     (hipStream_t)stream, A);
  return check_launch("k_move_poses");
}
