// apg_glimpse_poses.hip — glimpses, match scores and moves of the image envs at caller-chosen positions (gfx950).
//
//   k_glimpse_scores  for each position set m of M: K candidate positions on pool image index[m].  A unit (m, k) is
//                     the env's own glimpse (gs_axes / gs_pixels_t of apg_glimpse.hpp, the code k_glimpse_sep and the
//                     fused step run), and its score is np.mean((g - observed[m]) ** 2, axis=(-3, -2, -1)) in
//                     float32 as numpy evaluates it on a contiguous block: difference and square each rounded to
//                     f32 in element order, numpy's pairwise sum over the L = s0 * s1 * C values, (0 + sum) / L with
//                     a correctly rounded division (image_oracle.uniqueness's expression).
//   k_image_move      open-loop rollouts of candidate actions with the env's move (move_pos, as env_tail applies it).
//
// k_glimpse_scores, work assignment.  A 256-thread workgroup takes `upb` consecutive units of the flat [M * K] unit
// list (about four pixels per thread, as k_glimpse_sep), so its units may straddle position sets and the last
// workgroup is ragged.
//   * scores wanted: the glimpses of the units are computed into LDS [upb][L]; observed[m] of every set the units
//     touch (consecutive sets: one contiguous run of `observed`) is staged in LDS once per workgroup, not once per
//     candidate.  The glimpses are copied to global memory only when the glimpse output is requested.  The squared
//     differences then overwrite the LDS glimpses, and each leaf (a run of <= 128 values) of numpy's pairwise
//     recursion is summed by 8 lanes (pw_leaf8: lane j owns accumulator j); one thread per unit combines the leaves
//     in the recursion's order.  LDS: (upb + sets) * L floats + the axes, held under GP_LDS_BYTES (48 KiB, inside
//     the 64 KiB a launch gets without asking) by lowering upb; upb = 1 fits up to L = GP_MAX_SCORE_L = 4096.
//   * glimpses only: written straight to global memory (sensor sides <= 256, L <= MAX_PW_N as apg_image_glimpse).
// Domain.  A unit whose sampling coordinates leave the image (RGI bounds_error=True), or with a non-finite position,
// is NaN (score and glimpse) and ORs APG_ERR_OOB_X / APG_ERR_OOB_Y into err; so is a unit whose index is outside
// [0, pool_len) (APG_ERR_INDEX).  Such a unit never addresses the pool with its own position or index: its axes are
// computed at position (0, 0) of image 0 and the result is discarded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/apgym_capi.h"
#include "apg_glimpse.hpp"
#include "apg_host.hpp"
#include "apg_pairwise.hpp"

namespace apg {
namespace {

// (mirrored as GLIMPSE_SCORES_* / IMAGE_MOVE_MAX_T in ap_gym_amd/_native.py)
constexpr int GP_MAX_SCORE_L = 4096;    // values per glimpse the fused score takes
constexpr int GP_LDS_BYTES = 48 * 1024; // dynamic LDS of a k_glimpse_scores workgroup
constexpr int GP_MAX_LEAVES = 64;       // leaves of numpy's pairwise recursion over L <= 4096 (six split levels)
constexpr int GP_MAX_T = 4096;          // actions per candidate of k_image_move

struct ScoreArgs {
  GlimpseGeo g;
  const void *pool;
  const int64_t *index;
  const void *pos;
  const float *observed;
  float *score, *glimpse;
  uint32_t *err;
  int64_t pool_len;
  int units, k, upb, nsets_max, nleaves;
  FastDiv per_div, s1_div, side_div, l_div;
};

// the leaves' partial sums combined in the order of numpy's recursion (pw_sum: left, right, one add)
template <int DEPTH>
APG_DEV float pw_combine(const float *leaf, int &li, int n) {
  if constexpr (DEPTH == 0) {
    return leaf[li++];
  } else {
    if (n <= 128) return leaf[li++];
    int n2 = n / 2;
    n2 -= n2 % 8;
    const float a = pw_combine<DEPTH - 1>(leaf, li, n2);
    const float b = pw_combine<DEPTH - 1>(leaf, li, n - n2);
    return __fadd_rn(a, b);
  }
}

template <class PosT>
__global__ __launch_bounds__(GS_THREADS) void k_glimpse_scores(ScoreArgs A) {
  extern __shared__ double s_dyn[];  // Axis [upb][s0 + s1] | glimpses f32 [upb][L] | observed [sets][L] | leaf sums
  __shared__ float s_lut[256];
  __shared__ int64_t s_base[GS_MAX_UNITS];
  __shared__ uint32_t s_bad[GS_MAX_UNITS];
  __shared__ int s_set[GS_MAX_UNITS];
  __shared__ int s_loff[GP_MAX_LEAVES], s_llen[GP_MAX_LEAVES], s_stk[2][16];
  const GlimpseGeo &g = A.g;
  const int tid = threadIdx.x;
  const int L = g.s0 * g.s1 * g.c, side = g.s0 + g.s1;
  const int u0 = blockIdx.x * A.upb, nu = A.units - u0 < A.upb ? A.units - u0 : A.upb;
  const int m0 = u0 / A.k, nsets = (u0 + nu - 1) / A.k - m0 + 1;
  const bool fused = A.score != nullptr;
  Axis *s_ax = reinterpret_cast<Axis *>(s_dyn);
  float *s_g = reinterpret_cast<float *>(s_ax + (size_t)A.upb * side);
  float *s_o = s_g + (size_t)A.upb * L;
  float *s_leaf = s_o + (size_t)A.nsets_max * L;
  const PosT *pos = static_cast<const PosT *>(A.pos);
  const float nanv = __builtin_nanf("");

  if (!APG_U8_ARITH) for (int v = tid; v < 256; v += GS_THREADS) s_lut[v] = u8_value((unsigned)v);
  if (tid < nu) {
    const int m = (u0 + tid) / A.k;
    const int64_t idx = A.index[m];
    const bool ok = idx >= 0 && idx < A.pool_len;  // an index outside the pool is never used to address it
    s_base[tid] = ok ? idx * g.img_elems : 0;
    s_bad[tid] = ok ? 0u : APG_ERR_INDEX;
    s_set[tid] = m - m0;
  }
  if (fused) {
    // observed[m0 .. m0 + nsets): one contiguous run, read once for all the candidates of the workgroup
    const float *src = A.observed + (size_t)m0 * L;
    for (int i = tid; i < nsets * L; i += GS_THREADS) s_o[i] = src[i];
    if (tid == 0) {  // the leaves of numpy's pairwise recursion over L, in order (an explicit stack: left first)
      int sp = 1, nl = 0;
      s_stk[0][0] = 0;
      s_stk[1][0] = L;
      while (sp > 0) {
        sp--;
        const int o = s_stk[0][sp], n = s_stk[1][sp];
        if (n <= 128) {
          s_loff[nl] = o;
          s_llen[nl] = n;
          nl++;
        } else {
          int n2 = n / 2;
          n2 -= n2 % 8;
          s_stk[0][sp] = o + n2;
          s_stk[1][sp] = n - n2;
          s_stk[0][sp + 1] = o;
          s_stk[1][sp + 1] = n2;
          sp += 2;
        }
      }
    }
  }
  __syncthreads();
  // The bounds test of every sampling coordinate (the coordinate as gs_axes forms it: flip(denormalize(pos)) +
  // offsets); a NaN fails both comparisons.  The pixel values themselves come from gs_axes / gs_pixels_t alone.
  for (int q = tid; q < nu * side; q += GS_THREADS) {
    const int u = (int)A.side_div.div((uint32_t)q), k = q - u * side;
    const bool row = k < g.s0;
    const int t = row ? k : k - g.s0;
    const double p = (double)pos[2 * (size_t)(u0 + u) + (row ? 1 : 0)];
    const double off = __dmul_rn(__dsub_rn((double)t, ((double)(row ? g.s0 : g.s1) - 1.0) / 2.0), g.scale);
    const double c = __dadd_rn(__dmul_rn(p, row ? g.lim_y : g.lim_x), off);
    const double lim = row ? g.cy : g.cx;
    if (!(c >= -lim && c <= lim)) atomicOr(&s_bad[u], row ? APG_ERR_OOB_Y : APG_ERR_OOB_X);
  }
  __syncthreads();
  gs_axes(g, nullptr, [&](int u, int c) { return s_bad[u] ? 0.0 : (double)pos[2 * (size_t)(u0 + u) + c]; }, u0, nu, 1,
          A.side_div, s_ax, s_base);
  __syncthreads();
  if (!fused) {
    // glimpses only: straight to global memory, then NaN over the units outside the domain (same workgroup, after
    // the barrier: the later store wins)
    gs_pixels(g, A.pool, u0, nu, A.per_div, A.s1_div, s_ax, s_base, s_lut, A.glimpse);
    __syncthreads();
    float *dst = A.glimpse + (size_t)u0 * L;
    for (int i = tid; i < nu * L; i += GS_THREADS)
      if (s_bad[A.l_div.div((uint32_t)i)]) dst[i] = nanv;
  } else {
    gs_pixels(g, A.pool, 0, nu, A.per_div, A.s1_div, s_ax, s_base, s_lut, s_g);
    __syncthreads();
    float *dst = A.glimpse ? A.glimpse + (size_t)u0 * L : nullptr;
    for (int i = tid; i < nu * L; i += GS_THREADS) {
      const int u = (int)A.l_div.div((uint32_t)i), l = i - u * L;
      const float v = s_bad[u] ? nanv : s_g[i];
      if (dst) dst[i] = v;
      const float d = __fsub_rn(v, s_o[s_set[u] * L + l]);
      s_g[i] = __fmul_rn(d, d);
    }
    __syncthreads();
    // leaf sums: 8 lanes per (unit, leaf); every lane of a group takes the same branch of pw_leaf8
    const int j = tid & 7, nleaves = A.nleaves, tasks = nu * nleaves;
    for (int base = 0; base < tasks; base += GS_THREADS / 8) {
      const int task = base + (tid >> 3);
      const bool live = task < tasks;
      const int u = live ? task / nleaves : 0, lf = live ? task - u * nleaves : 0;
      const float r = pw_leaf8(s_g + (size_t)u * L, s_loff[lf], live ? s_llen[lf] : 0, j);
      if (live && j == 0) s_leaf[task] = r;
    }
    __syncthreads();
    if (tid < nu) {
      int li = 0;
      const float total = pw_combine<MAX_PW_DEPTH>(s_leaf + tid * nleaves, li, L);
      const float mean = f32_div(__fadd_rn(0.0f, total), (float)L);
      A.score[u0 + tid] = s_bad[tid] ? nanv : mean;
    }
  }
  if (tid < nu && s_bad[tid] && A.err) atomicOr(A.err, s_bad[tid]);
}

struct MoveArgs {
  const double *start;
  const float *actions;
  double *pos;
  float *glimpse_pos, *base_reward;
  uint32_t *err;
  double msl[2];
  int64_t units;
  int k, t, max_steps;
};

// One thread per candidate (m, k): move_pos applied T times from start[m], as env_tail does it.
__global__ __launch_bounds__(256) void k_image_move(MoveArgs A) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.units) return;
  EnvArgs a{};
  a.msl[0] = A.msl[0];
  a.msl[1] = A.msl[1];
  const int64_t m = c / A.k;
  double px = A.start[2 * m], py = A.start[2 * m + 1];
  const float *act = A.actions + 2 * (size_t)c * A.t;
  double *o_pos = A.pos + 2 * (size_t)c * A.t;
  float *o_gp = A.glimpse_pos + 2 * (size_t)c * A.t, *o_br = A.base_reward + (size_t)c * A.t;
  const float nanv = __builtin_nanf("");
  bool bad = false;
  for (int t = 0; t < A.t; t++) {
    float base = 0.0f;  // after max_steps actions the pose repeats and the base reward is 0
    if (t < A.max_steps) {
      const float a0 = act[2 * t], a1 = act[2 * t + 1];
      if (a0 != a0 || a1 != a1) bad = true;
      const float mag = move_pos(a, a0, a1, px, py);
      base = __fmul_rn(-mag, 1e-3f);  // -norm(action) * 1e-3 (f32)
    }
    if (bad) {  // a NaN action: NaN from that action on
      px = py = (double)nanv;
      base = nanv;
    }
    o_pos[2 * t] = px;
    o_pos[2 * t + 1] = py;
    o_gp[2 * t] = (float)px;
    o_gp[2 * t + 1] = (float)py;
    o_br[t] = base;
  }
  if (bad && A.err) atomicOr(A.err, APG_ERR_NAN_ACTION);
}

int pw_leaf_count(int n) {
  if (n <= 128) return 1;
  int n2 = n / 2;
  n2 -= n2 % 8;
  return pw_leaf_count(n2) + pw_leaf_count(n - n2);
}

}  // namespace
}  // namespace apg

extern "C" int apg_image_glimpse_scores(const apg_image_config *c, const void *pool, const int64_t *index,
                                        const void *pos, int pos_is_f32, int64_t m, int32_t k, const float *observed,
                                        float *score, float *glimpse, uint32_t *err, apg_stream_t stream) {
  using namespace apg;
  if (!c) return fail(APG_E_INVALID, "glimpse_scores: null config");
  if (int rc = validate(c)) return rc;
  if (m < 0 || k < 0) return fail(APG_E_INVALID, "glimpse_scores: m and k must be >= 0");
  if (!score && !glimpse) return fail(APG_E_INVALID, "glimpse_scores: neither score nor glimpse requested");
  if (score && !observed) return fail(APG_E_INVALID, "glimpse_scores: score needs observed");
  if (c->sensor_h > GS_MAX_SIDE || c->sensor_w > GS_MAX_SIDE)
    return fail(APG_E_INVALID, "glimpse_scores: sensor sides must be <= 256");
  GlimpseGeo g = make_geo(c);
  const int per = g.s0 * g.s1, L = per * g.c, side = g.s0 + g.s1;
  if (score && L > GP_MAX_SCORE_L)
    return fail(APG_E_INVALID, "glimpse_scores: the fused score takes glimpses of at most 4096 values "
                               "(sensor_h * sensor_w * channels); take the glimpses alone and score them outside");
  if (k > 0 && m > (((int64_t)1 << 31) - 1) / ((int64_t)k * per))
    return fail(APG_E_INVALID, "glimpse_scores: batch too large (>= 2**31 pixels)");
  if (m == 0 || k == 0) return APG_OK;
  if (!pool || !index || !pos) return fail(APG_E_INVALID, "glimpse_scores: null pool / index / pos");
  ScoreArgs A{};
  A.nleaves = score ? pw_leaf_count(L) : 0;
  if (A.nleaves > GP_MAX_LEAVES) return fail(APG_E_INVALID, "glimpse_scores: too many pairwise leaves");
  int upb = fastdiv_safe_units(glimpse_units_per_block(per), g.s0, g.s1);
  auto sets_of = [&](int u) { return (u + k - 2) / k + 1; };  // position sets that u consecutive units can touch
  auto lds_of = [&](int u) {
    size_t b = (size_t)u * side * sizeof(Axis);
    if (score) b += ((size_t)u * L + (size_t)sets_of(u) * L + (size_t)u * A.nleaves) * sizeof(float);
    return b;
  };
  while (upb > 1 && (lds_of(upb) > (size_t)GP_LDS_BYTES || !fastdiv_exact((uint32_t)L, (uint64_t)upb * L - 1))) upb--;
  if (lds_of(upb) > (size_t)GP_LDS_BYTES) return fail(APG_E_INVALID, "glimpse_scores: glimpse too large for LDS");
  A.g = g;
  A.pool = pool;
  A.index = index;
  A.pos = pos;
  A.observed = observed;
  A.score = score;
  A.glimpse = glimpse;
  A.err = err;
  A.pool_len = c->pool_len;
  A.units = (int)(m * k);
  A.k = k;
  A.upb = upb;
  A.nsets_max = score ? sets_of(upb) : 0;
  A.per_div = make_fastdiv((uint32_t)per);
  A.s1_div = make_fastdiv((uint32_t)g.s1);
  A.side_div = make_fastdiv((uint32_t)side);
  A.l_div = make_fastdiv((uint32_t)L);
  const dim3 grid((unsigned)((A.units + upb - 1) / upb));
  if (pos_is_f32)
    hipLaunchKernelGGL(k_glimpse_scores<float>, grid, dim3(GS_THREADS), lds_of(upb), (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(k_glimpse_scores<double>, grid, dim3(GS_THREADS), lds_of(upb), (hipStream_t)stream, A);
  return check_launch("k_glimpse_scores");
}

extern "C" int apg_image_move(const apg_image_config *c, const double *start, const float *actions, int64_t m,
                              int32_t k, int32_t t, int32_t max_steps, double *pos, float *glimpse_pos,
                              float *base_reward, uint32_t *err, apg_stream_t stream) {
  using namespace apg;
  if (!c) return fail(APG_E_INVALID, "image_move: null config");
  if (m < 0 || k < 0) return fail(APG_E_INVALID, "image_move: m and k must be >= 0");
  if (t < 1 || t > GP_MAX_T) return fail(APG_E_INVALID, "image_move: t must be in [1, 4096]");
  if (max_steps < 0) return fail(APG_E_INVALID, "image_move: max_steps must be >= 0");
  if (m == 0 || k == 0) return APG_OK;
  if (!start || !actions || !pos || !glimpse_pos || !base_reward)
    return fail(APG_E_INVALID, "image_move: null start / actions / pos / glimpse_pos / base_reward");
  if (k > 0 && m > (((int64_t)1 << 31) - 1) / k)
    return fail(APG_E_INVALID, "image_move: too many candidates (>= 2**31)");
  MoveArgs A{};
  A.start = start;
  A.actions = actions;
  A.pos = pos;
  A.glimpse_pos = glimpse_pos;
  A.base_reward = base_reward;
  A.err = err;
  A.msl[0] = c->max_step[0];
  A.msl[1] = c->max_step[1];
  A.units = m * k;
  A.k = k;
  A.t = t;
  A.max_steps = max_steps;
  hipLaunchKernelGGL(k_image_move, dim3((unsigned)((A.units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
  return check_launch("k_image_move");
}
