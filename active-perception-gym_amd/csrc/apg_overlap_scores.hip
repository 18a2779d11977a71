// apg_overlap_scores.hip — k_overlap_scores: how well a localization env's glimpse and target glimpse agree where
// the two sensor windows overlap under hypotheses of the target position, with a fused log-weight update (gfx950).
// The definition, step by step, is the comment of apg_image_overlap_scores in include/apgym_capi.h; this file restates
// only what the work split adds.
//
// Work assignment.  A 256-thread workgroup takes one set m and `chunk` consecutive hypotheses of it
// (apg_image_overlap_chunk: 64, halved down to 8 while the launch has fewer than OV_FILL_WGS workgroups, so one env
// with 4096 hypotheses still makes 512 workgroups).
//   phase 1  one thread per hypothesis: the shift, the domain and the overlap rectangle, all in f64 registers.  A
//            hypothesis with count = 0 (non-finite, no overlap) is finished here, its outputs written, without a
//            single LDS or glimpse read; the others are listed.  A workgroup that lists none ends here: on a belief
//            grid most hypotheses lie further than a sensor width from the glimpse, so most workgroups read 16 bytes
//            of q and their hypotheses and nothing else.
//   phase 2  g[m] and G[m] are staged in LDS once (2 L floats, <= 32 KiB).  A task is a (listed hypothesis, leaf of
//            numpy's pairwise recursion over L) pair, taken by a group of 8 lanes as in k_glimpse_scores: lane j owns
//            accumulator j of the leaf (ov_leaf8, pw_leaf8 of apg_glimpse.hpp with the squared error computed on the
//            fly in place of an LDS read).  A leaf whose rows all lie outside the overlap is +0.0 without a read.
//   phase 3  one thread per listed hypothesis combines its leaves in the recursion's order and writes the outputs.
// LDS: 2 L floats + chunk * leaves floats (<= 32 + 16 KiB dynamic) + 3.4 KiB static, inside the 64 KiB a launch
// gets without asking.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/apgym_capi.h"
#include "apg_glimpse.hpp"
#include "apg_host.hpp"
#include "apg_pairwise.hpp"

namespace apg {
namespace {

// (mirrored as OVERLAP_SCORES_* in ap_gym_amd/_native.py)
constexpr int OV_THREADS = 256;
constexpr int OV_MAX_L = 4096;      // values per glimpse (GLIMPSE_SCORES_MAX_L)
constexpr int OV_MAX_LEAVES = 64;   // leaves of numpy's pairwise recursion over L <= 4096
constexpr int OV_MAX_CHUNK = 64;    // hypotheses per workgroup, at most
constexpr int OV_MIN_CHUNK = 8;     // ... and at least (unless k is smaller)
constexpr int OV_FILL_WGS = 1024;   // the chunk is halved while the launch has fewer workgroups than this

struct OvArgs {
  const float *g, *tg, *logw;
  const void *q, *h;
  float *sse, *logw_out;
  int32_t *count;
  uint32_t *err;
  double lim_x, lim_y, scale;
  float gain, tau;
  int k, chunk, cps;  // hypotheses per set, per workgroup; workgroups per set
  int s0, s1, c, L, nleaves;
  int q_f32, h_f32, h_shared;
  FastDiv row_div, c_div;  // by s1 * c, by c (n < L <= 4096: exact for every divisor)
};

struct Hyp {  // a listed hypothesis: its index in the chunk, the shift's integer and fractional parts, the overlap
  int t, iy, ix, a_lo, a_hi, b_lo, b_hi, count;
  float fy, fx;
};

// the leaves' partial sums combined in the order of numpy's recursion (k_glimpse_scores' pw_combine)
template <int DEPTH>
APG_DEV float ov_combine(const float *leaf, int &li, int n) {
  if constexpr (DEPTH == 0) {
    return leaf[li++];
  } else {
    if (n <= 128) return leaf[li++];
    int n2 = n / 2;
    n2 -= n2 % 8;
    const float a = ov_combine<DEPTH - 1>(leaf, li, n2);
    const float b = ov_combine<DEPTH - 1>(leaf, li, n - n2);
    return __fadd_rn(a, b);
  }
}

// pw_leaf8 (apg_glimpse.hpp) over values x(i) computed on the fly: numpy's pairwise leaf of x(off .. off + n) by the
// 8 lanes of a group, lane j owning accumulator j; every lane of a group takes the same path and gets the result
template <class X>
APG_DEV float ov_leaf8(const X &x, int off, int n, int j) {
  if (n < 8) {
    float r = 0.0f;
    for (int i = 0; i < n; i++) r = __fadd_rn(r, x(off + i));
    return r;
  }
  float r = x(off + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8) r = __fadd_rn(r, x(off + i + j));
  const int g0 = (int)(threadIdx.x & 63u) & ~7;
  float q[8];
#pragma unroll
  for (int k = 0; k < 8; k++) q[k] = __shfl(r, g0 + k, 64);
  float res = __fadd_rn(__fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3])),
                        __fadd_rn(__fadd_rn(q[4], q[5]), __fadd_rn(q[6], q[7])));
  for (; i < n; i++) res = __fadd_rn(res, x(off + i));
  return res;
}

// The indices t of 0..n-1 with 0 <= t + d <= n - 1 in f64 (the sum rounded once): t + d is nondecreasing in t, so
// they form one range [lo, hi] (empty: lo > hi).  |d| < n <= 4096.
APG_DEV void overlap_range(double d, int n, int &lo, int &hi) {
  const double top = (double)(n - 1);
  lo = (int)ceil(-d);
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  while (lo > 0 && __dadd_rn((double)(lo - 1), d) >= 0.0) lo--;
  while (lo < n && !(__dadd_rn((double)lo, d) >= 0.0)) lo++;
  hi = (int)floor(__dsub_rn(top, d));
  hi = hi > n - 1 ? n - 1 : (hi < -1 ? -1 : hi);
  while (hi < n - 1 && __dadd_rn((double)(hi + 1), d) <= top) hi++;
  while (hi >= 0 && !(__dadd_rn((double)hi, d) <= top)) hi--;
}

APG_DEV double load_pos(const void *p, size_t i, int is_f32) {
  return is_f32 ? (double)static_cast<const float *>(p)[i] : static_cast<const double *>(p)[i];
}

APG_DEV bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and +-inf

// step 6 of the definition
APG_DEV float belief_update(float logw, float gain, float tau, int count, float sse) {
  if (!(fabsf(sse) <= 3.4028234663852886e38f)) return __builtin_nanf("");
  return __fadd_rn(logw, __fmul_rn(gain, __fsub_rn(__fmul_rn(tau, (float)count), sse)));
}

__global__ __launch_bounds__(OV_THREADS) void k_overlap_scores(OvArgs A) {
  extern __shared__ float s_dyn[];  // g [L] | G [L] | leaf sums [chunk][nleaves]
  __shared__ Hyp s_hyp[OV_MAX_CHUNK];
  __shared__ int s_loff[OV_MAX_LEAVES], s_llen[OV_MAX_LEAVES], s_stk[2][16];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  const int L = A.L, s0 = A.s0, s1 = A.s1, C = A.c;
  const int64_t m = blockIdx.x / (unsigned)A.cps;
  const int k0 = (int)(blockIdx.x - (unsigned)m * (unsigned)A.cps) * A.chunk;
  const int nk = A.k - k0 < A.chunk ? A.k - k0 : A.chunk;
  float *s_g = s_dyn, *s_tg = s_dyn + L, *s_leaf = s_dyn + 2 * L;
  const float nanv = __builtin_nanf("");
  const bool fused = A.logw != nullptr;

  if (tid == 0) s_n = 0;
  __syncthreads();
  // ---- phase 1: the shift, the domain and the overlap rectangle of hypothesis k0 + tid
  bool bad = false;
  if (tid < nk) {
    const size_t out = (size_t)m * A.k + k0 + tid;
    const size_t hi_ = 2 * ((A.h_shared ? (size_t)0 : (size_t)m * A.k) + k0 + tid);
    const double qx = load_pos(A.q, 2 * (size_t)m, A.q_f32), qy = load_pos(A.q, 2 * (size_t)m + 1, A.q_f32);
    const double hx = load_pos(A.h, hi_, A.h_f32), hy = load_pos(A.h, hi_ + 1, A.h_f32);
    float sse = 0.0f;
    bool listed = false;
    if (!(finite_f64(qx) && finite_f64(qy) && finite_f64(hx) && finite_f64(hy))) {
      sse = nanv;
      bad = true;
    } else {
      const double dx = __ddiv_rn(__dmul_rn(__dsub_rn(qx, hx), A.lim_x), A.scale);
      const double dy = __ddiv_rn(__dmul_rn(__dsub_rn(qy, hy), A.lim_y), A.scale);
      if (fabs(dy) < (double)s0 && fabs(dx) < (double)s1) {
        Hyp hp;
        overlap_range(dy, s0, hp.a_lo, hp.a_hi);
        overlap_range(dx, s1, hp.b_lo, hp.b_hi);
        if (hp.a_lo <= hp.a_hi && hp.b_lo <= hp.b_hi) {
          const double fly = floor(dy), flx = floor(dx);
          hp.t = tid;
          hp.iy = (int)fly;
          hp.ix = (int)flx;
          hp.fy = (float)__dsub_rn(dy, fly);
          hp.fx = (float)__dsub_rn(dx, flx);
          hp.count = C * (hp.a_hi - hp.a_lo + 1) * (hp.b_hi - hp.b_lo + 1);
          s_hyp[atomicAdd(&s_n, 1)] = hp;  // (the order of the list does not reach any result)
          listed = true;
        }
      }
    }
    if (!listed) {  // count = 0: finished here
      A.sse[out] = sse;
      A.count[out] = 0;
      if (fused) A.logw_out[out] = belief_update(A.logw[out], A.gain, A.tau, 0, sse);
    }
  }
  if (__syncthreads_or(bad) && tid == 0 && A.err) atomicOr(A.err, APG_ERR_BAD_POSE);
  const int nlist = s_n;
  if (nlist == 0) return;  // (uniform: s_n was read after the barrier)

  // ---- phase 2: g[m], G[m] into LDS; the leaves of numpy's pairwise recursion over L, in order
  {
    const float *gs = A.g + (size_t)m * L, *ts = A.tg + (size_t)m * L;
    for (int i = tid; i < L; i += OV_THREADS) {
      s_g[i] = gs[i];
      s_tg[i] = ts[i];
    }
    if (tid == 0) {
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
  const int j = tid & 7, nleaves = A.nleaves, tasks = nlist * nleaves, rowlen = s1 * C;
  for (int base = 0; base < tasks; base += OV_THREADS / 8) {
    const int task = base + (tid >> 3);
    const bool live = task < tasks;
    const int u = live ? task / nleaves : 0, lf = live ? task - u * nleaves : 0;
    const Hyp hp = s_hyp[u];
    const int off = s_loff[lf];
    int n = live ? s_llen[lf] : 0;
    // rows of the leaf: all outside the overlap -> every e is +0.0 and so is their sum
    if (live && ((int)A.row_div.div((uint32_t)(off + n - 1)) < hp.a_lo || (int)A.row_div.div((uint32_t)off) > hp.a_hi))
      n = 0;
    const float nfy = __fsub_rn(1.0f, hp.fy), nfx = __fsub_rn(1.0f, hp.fx);
    auto e = [&](int i) -> float {
      const int a = (int)A.row_div.div((uint32_t)i), rem = i - a * rowlen;
      const int b = (int)A.c_div.div((uint32_t)rem), ch = rem - b * C;
      if (a < hp.a_lo || a > hp.a_hi || b < hp.b_lo || b > hp.b_hi) return 0.0f;
      // in the overlap r0 and c0 are inside the glimpse by construction; the clamps keep every LDS address inside
      // the block whatever the inputs hold
      int r0 = a + hp.iy, c0 = b + hp.ix;
      r0 = r0 < 0 ? 0 : (r0 > s0 - 1 ? s0 - 1 : r0);
      c0 = c0 < 0 ? 0 : (c0 > s1 - 1 ? s1 - 1 : c0);
      const int r1 = r0 + 1 < s0 ? r0 + 1 : s0 - 1, c1 = c0 + 1 < s1 ? c0 + 1 : s1 - 1;
      const float t00 = s_tg[(r0 * s1 + c0) * C + ch], t01 = s_tg[(r0 * s1 + c1) * C + ch];
      const float t10 = s_tg[(r1 * s1 + c0) * C + ch], t11 = s_tg[(r1 * s1 + c1) * C + ch];
      const float top = __fadd_rn(__fmul_rn(t00, nfx), __fmul_rn(t01, hp.fx));
      const float bot = __fadd_rn(__fmul_rn(t10, nfx), __fmul_rn(t11, hp.fx));
      const float pred = __fadd_rn(__fmul_rn(top, nfy), __fmul_rn(bot, hp.fy));
      const float d = __fsub_rn(s_g[i], pred);
      return __fmul_rn(d, d);
    };
    const float r = ov_leaf8(e, off, n, j);
    if (live && j == 0) s_leaf[task] = r;
  }
  __syncthreads();
  // ---- phase 3: the leaves combined, the outputs of the listed hypotheses
  if (tid < nlist) {
    int li = 0;
    const float sse = ov_combine<MAX_PW_DEPTH>(s_leaf + tid * nleaves, li, L);
    const Hyp hp = s_hyp[tid];
    const size_t out = (size_t)m * A.k + k0 + hp.t;
    A.sse[out] = sse;
    A.count[out] = hp.count;
    if (fused) A.logw_out[out] = belief_update(A.logw[out], A.gain, A.tau, hp.count, sse);
  }
}

int ov_leaf_count(int n) {
  if (n <= 128) return 1;
  int n2 = n / 2;
  n2 -= n2 % 8;
  return ov_leaf_count(n2) + ov_leaf_count(n - n2);
}

int ov_chunk(int64_t m, int32_t k) {
  if (m <= 0 || k <= 0) return 0;
  int chunk = OV_MAX_CHUNK;
  while (chunk > OV_MIN_CHUNK && m * ((k + chunk - 1) / chunk) < OV_FILL_WGS) chunk /= 2;
  return chunk;
}

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && pa < pb + nb && pb < pa + na;
}

}  // namespace
}  // namespace apg

extern "C" int32_t apg_image_overlap_chunk(int64_t m, int32_t k) { return apg::ov_chunk(m, k); }

extern "C" int apg_image_overlap_scores(const apg_overlap_scores_args *a, apg_stream_t stream) {
  using namespace apg;
  if (!a) return fail(APG_E_INVALID, "overlap_scores: null arguments");
  if (a->m < 0 || a->k < 0) return fail(APG_E_INVALID, "overlap_scores: m and k must be >= 0");
  if (a->height < 2 || a->width < 2) return fail(APG_E_INVALID, "overlap_scores: images must be at least 2 x 2");
  if (a->sensor_h < 1 || a->sensor_w < 1 || a->channels < 1)
    return fail(APG_E_INVALID, "overlap_scores: sensor sides and channels must be positive");
  if (!(a->sensor_scale > 0.0 && std::isfinite(a->sensor_scale)))
    return fail(APG_E_INVALID, "overlap_scores: sensor_scale must be positive and finite");
  const int64_t l64 = (int64_t)a->sensor_h * a->sensor_w * a->channels;
  if (a->sensor_h > OV_MAX_L || a->sensor_w > OV_MAX_L || a->channels > OV_MAX_L || l64 > OV_MAX_L)
    return fail(APG_E_INVALID, "overlap_scores: a glimpse holds at most 4096 values (sensor_h * sensor_w * channels)");
  if ((a->logw == nullptr) != (a->logw_out == nullptr))
    return fail(APG_E_INVALID, "overlap_scores: logw and logw_out go together (both or neither)");
  if (a->m == 0 || a->k == 0) return APG_OK;
  if (!a->glimpse || !a->target_glimpse || !a->glimpse_pos || !a->hypotheses || !a->sse || !a->count)
    return fail(APG_E_INVALID,
                "overlap_scores: null glimpse / target_glimpse / glimpse_pos / hypotheses / sse / count");
  const int L = (int)l64, chunk = ov_chunk(a->m, a->k), cps = (a->k + chunk - 1) / chunk;
  if (a->m > (((int64_t)1 << 31) - 1) / cps)
    return fail(APG_E_INVALID, "overlap_scores: too many workgroups (m * ceil(k / chunk) >= 2**31): split the sets");
  const size_t mk = (size_t)a->m * a->k;
  if (a->logw_out != a->logw && ranges_overlap(a->logw_out, 4 * mk, a->logw, 4 * mk))
    return fail(APG_E_INVALID, "overlap_scores: logw_out overlaps logw partially (it may be exactly logw)");
  if (ranges_overlap(a->sse, 4 * mk, a->count, 4 * mk) || ranges_overlap(a->sse, 4 * mk, a->logw_out, 4 * mk) ||
      ranges_overlap(a->count, 4 * mk, a->logw_out, 4 * mk) || ranges_overlap(a->sse, 4 * mk, a->logw, 4 * mk) ||
      ranges_overlap(a->count, 4 * mk, a->logw, 4 * mk))
    return fail(APG_E_INVALID, "overlap_scores: sse, count and logw_out must not overlap each other or logw");
  // sensor_pos_lim_pixels as the glimpse kernels form it (make_geo, apg_glimpse.hpp)
  apg_image_config c{};
  c.height = a->height;
  c.width = a->width;
  c.sensor_h = a->sensor_h;
  c.sensor_w = a->sensor_w;
  c.channels = c.pool_channels = a->channels;
  c.sensor_scale = a->sensor_scale;
  const GlimpseGeo geo = make_geo(&c);
  OvArgs A{};
  A.g = a->glimpse;
  A.tg = a->target_glimpse;
  A.logw = a->logw;
  A.q = a->glimpse_pos;
  A.h = a->hypotheses;
  A.sse = a->sse;
  A.logw_out = a->logw_out;
  A.count = a->count;
  A.err = a->err;
  A.lim_x = geo.lim_x;
  A.lim_y = geo.lim_y;
  A.scale = a->sensor_scale;
  A.gain = a->gain;
  A.tau = a->tau;
  A.k = a->k;
  A.chunk = chunk;
  A.cps = cps;
  A.s0 = a->sensor_h;
  A.s1 = a->sensor_w;
  A.c = a->channels;
  A.L = L;
  A.nleaves = ov_leaf_count(L);
  if (A.nleaves > OV_MAX_LEAVES) return fail(APG_E_INVALID, "overlap_scores: too many pairwise leaves");
  A.q_f32 = a->pos_is_f32 != 0;
  A.h_f32 = a->hyp_is_f32 != 0;
  A.h_shared = a->hyp_shared != 0;
  A.row_div = make_fastdiv((uint32_t)(a->sensor_w * a->channels));
  A.c_div = make_fastdiv((uint32_t)a->channels);
  const size_t lds = ((size_t)2 * L + (size_t)chunk * A.nleaves) * sizeof(float);
  hipLaunchKernelGGL(k_overlap_scores, dim3((unsigned)(a->m * cps)), dim3(OV_THREADS), lds, (hipStream_t)stream, A);
  return check_launch("k_overlap_scores");
}
